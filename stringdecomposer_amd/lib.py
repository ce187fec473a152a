"""ctypes binding of libsd_hip.so (include/sd_hip.h).

This is the call that replaces the reference's subprocess boundary
(stringdecomposer/main.py:194: subprocess.run([SD_BIN, ...], stdout=raw_file)).  The library has
no CPU fallback; a missing library or a missing GPU is a loud error.
"""
import ctypes as C
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
# SD_HIP_LIB lets a developer A/B an alternative build of the same library (never a CPU path)
LIB_PATH = os.environ.get("SD_HIP_LIB") or os.path.join(HERE, "csrc", "libsd_hip.so")

SD_OK = 0
SD_ERR_IO = 2
SD_ERR_FORMAT = 3
SD_ERR_PARAM = 4
SD_ERR_EMPTY = 6
SD_ERR_INTERNAL = 7
SD_ERR_NO_DEVICE = 8
SD_ERR_UNSUPPORTED = 9
SD_ERR_HIP = 10
SD_ERR_SYMBOL = 255

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_FAST = 0, 1, 2

EXPORTS = [
    "sd_pipeline_logic_selftest",
    "sd_params_default", "sd_version", "sd_device_count", "sd_free", "sd_decompose_files",
    "sd_decompose", "sd_engine_create", "sd_engine_destroy", "sd_engine_load_reads",
    "sd_engine_run", "sd_engine_fetch", "sd_engine_assemble", "sd_engine_timings",
    "sd_engine_info", "sd_chunk_plan", "sd_seam_merge", "sd_format_rows", "sd_fasta_load",
    "sd_fasta_free", "sd_nw_identity_batch", "sd_identity_segments", "sd_chunk_table_size",
    "sd_decompose_chunk_range", "sd_assemble_tsv", "sd_release_cache", "sd_format_alt_rows",
    "sd_stream_create", "sd_stream_destroy", "sd_stream_submit", "sd_stream_collect", "sd_stream_stats",
    "sd_stream_info", "sd_pack_bases", "sd_identity_segments_dev", "sd_nw_release_cache", "sd_last_run_stats", "sd_guard_trips",
    "sd_nw_route_counts",
    "sd_run_files", "sd_convert_raw_tsv", "sd_decompose_files_range", "sd_assemble_files_tsv",
    "sd_host_stage_rates", "sd_run_files_range", "sd_plan_info", "sd_write_parts_selftest", "sd_convert_raw_tsv_range",
    "sd_write_records", "sd_read_records", "sd_records_free", "sd_records_to_raw_tsv", "sd_decompose_files_records",
    "sd_run_files_records",
    "sd_range_assemble_begin", "sd_range_assemble_begin_files", "sd_range_assemble_text", "sd_range_assemble_write",
    "sd_range_assemble_copy", "sd_range_assemble_stats", "sd_range_assemble_free", "sd_decompose_files_range_begin",
    "sd_range_assemble_records",
    "sd_run_files_devices", "sd_last_run_device_stats", "sd_multi_device_selftest",
    "sd_stream_create_final", "sd_stream_collect_final", "sd_stream_keys", "sd_stream_final_stats",
    "sd_stream_create_devices", "sd_stream_create_final_devices", "sd_stream_device_stats",
    "sd_profile_segments", "sd_profile_segments_dev", "sd_last_run_profile", "sd_stream_profile",
    "sd_stream_submit_dev", "sd_engine_load_reads_dev", "sd_pack_bases_dev", "sd_engine_filter_result",
    "sd_fasta_load_ex", "sd_normalize_host", "sd_normalize_dev", "sd_last_run_input_stats",
    "sd_stream_peek_dev", "sd_stream_collect_dev", "sd_engine_rows_dev", "sd_seam_merge_dev", "sd_seam_pieces_selftest",
    "sd_scan_selftest",
    "sd_stream_peek_final_dev", "sd_stream_collect_final_dev", "sd_final_select_dev", "sd_final_select_host",
    "sd_stream_profile_dev", "sd_stream_profile_stats", "sd_final_profile_dev", "sd_final_profile_host",
    "sd_plan_floor_levels",
    "sd_text_tables_create", "sd_text_tables_destroy", "sd_text_final_size_dev", "sd_text_final_write_dev",
    "sd_text_raw_size_dev", "sd_text_raw_write_dev", "sd_text_final_host", "sd_text_raw_host",
    "sd_msa_row_offsets", "sd_msa_segments", "sd_msa_segments_dev", "sd_msa_tables_create", "sd_msa_tables_destroy",
    "sd_msa_final_size_dev", "sd_msa_final_write_dev", "sd_msa_kernel_bench",
    "sd_lag_segments", "sd_lag_segments_dev", "sd_lag_final_dev", "sd_lag_final_host", "sd_lag_identities", "sd_lag_periods",
    "sd_lag_kernel_bench",
    "sd_heat_layout", "sd_heat_segments", "sd_heat_segments_dev", "sd_heat_final_dev", "sd_heat_final_host", "sd_heat_identities",
    "sd_heat_kernel_bench",
    "sd_autocorr_layout", "sd_autocorr_host", "sd_autocorr_dev", "sd_autocorr_reads_dev", "sd_autocorr_positions", "sd_autocorr_peaks",
    "sd_autocorr_seed", "sd_autocorr_info", "sd_autocorr_kernel_bench",
    "sd_motif_compile", "sd_motif_host", "sd_motif_dev", "sd_motif_reads_size_dev", "sd_motif_reads_write_dev", "sd_motif_info",
    "sd_motif_kernel_bench",
    "sd_motif_edit_host", "sd_motif_edit_dev", "sd_motif_edit_reads_size_dev", "sd_motif_edit_reads_write_dev", "sd_motif_edit_info",
    "sd_motif_edit_kernel_bench",
    "sd_cyclic_pairs_host", "sd_cyclic_pairs_dev", "sd_cyclic_merge_host", "sd_cyclic_merge_dev", "sd_cyclic_canon", "sd_cyclic_info",
    "sd_cyclic_kernel_bench", "sd_cyclic_pairs_team_host", "sd_cyclic_long_info", "sd_cyclic_long_kernel_bench",
    "sd_split_host", "sd_split_dev", "sd_split_final_host", "sd_split_info", "sd_split_kernel_bench",
    "sd_hor_rows", "sd_hor_final_host", "sd_hor_name", "sd_hor_info",
    "sd_dotplot_layout", "sd_dotplot_host", "sd_dotplot_dev", "sd_dotplot_reads_dev", "sd_dotplot_info", "sd_dotplot_hash", "sd_dotplot_kernel_bench",
    "sd_screen_create", "sd_screen_destroy", "sd_screen_set_general", "sd_screen_kernel", "sd_screen_chunks",
    "sd_screen_chunks_dev", "sd_screen_chunks_host", "sd_screen_regions", "sd_screen_kernel_ms", "sd_run_files_screen",
    "sd_screen_kernel_bench",
]


class SdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsd_hip rc=%d: %s" % (code, msg))
        self.code = code
        self.msg = msg


class Params(C.Structure):
    _fields_ = [("ins", C.c_int32), ("del_", C.c_int32), ("mismatch", C.c_int32),
                ("match", C.c_int32), ("part_size", C.c_int32), ("overlap", C.c_int32),
                ("ed_thr", C.c_int32), ("threads", C.c_int32), ("device", C.c_int32),
                ("kernel", C.c_int32), ("max_batch_rows", C.c_int32), ("reserved", C.c_int32 * 5)]


class Rec(C.Structure):
    _fields_ = [("tmpl", C.c_int32), ("start", C.c_int32), ("end", C.c_int32),
                ("score", C.c_int32)]


class FinalRec(C.Structure):
    """sd_final_row (include/sd_hip.h): one kept block of a final-mode stream."""
    _fields_ = [("read", C.c_int32), ("start", C.c_int64), ("end", C.c_int64), ("best", C.c_int32),
                ("second", C.c_int32), ("homo_best", C.c_int32), ("homo_second", C.c_int32), ("ident", C.c_double),
                ("second_ident", C.c_double), ("homo_ident", C.c_double), ("homo_second_ident", C.c_double),
                ("reliable", C.c_int8)]


class Records(C.Structure):
    """sd_records (include/sd_hip.h): a parsed binary record stream."""
    _fields_ = [("ins", C.c_int32), ("del_", C.c_int32), ("mismatch", C.c_int32), ("match", C.c_int32),
                ("part_size", C.c_int32), ("overlap", C.c_int32), ("ed_thr", C.c_int32),
                ("n_templates", C.c_int32), ("tmpl_names", C.POINTER(C.c_char_p)),
                ("n_reads", C.c_int32), ("read_names", C.POINTER(C.c_char_p)),
                ("read_lens", C.POINTER(C.c_int64)), ("row_off", C.POINTER(C.c_int64)),
                ("n_rows", C.c_int64), ("rows", C.POINTER(Rec))]


class Fasta(C.Structure):
    _fields_ = [("n", C.c_int32), ("names", C.POINTER(C.c_char_p)),
                ("seqs", C.POINTER(C.c_void_p)), ("lens", C.POINTER(C.c_int64)),
                ("has_n", C.c_int32)]


_lib = None


def load():
    """Load libsd_hip.so.  Raises (never silently falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise SdError(SD_ERR_INTERNAL,
                      "%s is missing: build it with `make -C stringdecomposer_amd/csrc` "
                      "(or python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.sd_params_default.argtypes = [P(Params)]
    L.sd_version.restype = C.c_char_p
    L.sd_device_count.restype = C.c_int
    L.sd_free.argtypes = [C.c_void_p]
    L.sd_decompose_files.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_char_p, C.c_char_p, C.c_size_t]
    L.sd_decompose.argtypes = [P(C.c_char_p), P(C.c_char_p), P(C.c_int64), C.c_int32, P(C.c_char_p),
                               P(C.c_char_p), P(C.c_int32), C.c_int32, P(Params), P(C.c_void_p),
                               P(C.c_size_t), C.c_char_p, C.c_size_t]
    L.sd_engine_create.argtypes = [P(C.c_void_p), P(Params), P(C.c_char_p), P(C.c_int32), C.c_int32,
                                   C.c_char_p, C.c_size_t]
    L.sd_engine_destroy.argtypes = [C.c_void_p]
    L.sd_engine_load_reads.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_int64), C.c_int32,
                                       P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_engine_run.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_engine_fetch.argtypes = [C.c_void_p, P(P(Rec)), P(P(C.c_int64)), C.c_char_p, C.c_size_t]
    L.sd_engine_assemble.argtypes = [C.c_void_p, P(Rec), P(C.c_int64), P(P(Rec)), P(P(C.c_int64)),
                                     C.c_char_p, C.c_size_t]
    L.sd_engine_timings.argtypes = [C.c_void_p, P(C.c_float)]
    L.sd_engine_info.argtypes = [C.c_void_p, P(C.c_int64)]
    L.sd_plan_info.argtypes = [P(Params), P(C.c_char_p), P(C.c_int32), C.c_int32, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_plan_floor_levels.argtypes = [P(Params), P(C.c_char_p), P(C.c_int32), C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                       P(C.c_int32), C.c_int64, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_chunk_plan.restype = C.c_int32
    L.sd_chunk_plan.argtypes = [C.c_int64, C.c_int32, C.c_int32, P(C.c_int64), P(C.c_int32), C.c_int32]
    L.sd_seam_merge.restype = C.c_int32
    L.sd_seam_merge.argtypes = [P(Rec), C.c_int32]
    L.sd_format_rows.argtypes = [C.c_char_p, P(C.c_char_p), P(Rec), C.c_int32, P(C.c_void_p), P(C.c_size_t)]
    L.sd_fasta_load.argtypes = [C.c_char_p, P(Fasta), C.c_char_p, C.c_size_t]
    L.sd_fasta_load_ex.argtypes = [C.c_char_p, C.c_int32, P(Fasta), C.c_char_p, C.c_size_t]
    L.sd_fasta_free.argtypes = [P(Fasta)]
    L.sd_normalize_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sd_normalize_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_last_run_input_stats.argtypes = [P(C.c_int64)]
    L.sd_last_run_input_stats.restype = None
    L.sd_nw_identity_batch.argtypes = [P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(C.c_int32),
                                       C.c_int64, C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    L.sd_identity_segments.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                       P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_identity_segments_dev.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                           P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_run_files.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32,
                               C.c_int32, P(C.c_double), C.c_char_p, C.c_size_t]
    L.sd_run_files_range.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_int32, C.c_int32, C.c_char_p, C.c_char_p,
                                     C.c_char_p, C.c_int32, C.c_int32, P(C.c_double), P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_convert_raw_tsv.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32,
                                     P(C.c_double), C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sd_decompose_files_range.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_int32, C.c_int32, P(P(Rec)),
                                           P(P(C.c_int64)), P(C.c_int64), P(C.c_int64), P(C.c_int64), C.c_char_p,
                                           C.c_size_t]
    L.sd_assemble_files_tsv.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_char_p, C.c_char_p, C.c_size_t]
    L.sd_host_stage_rates.argtypes = [P(C.c_char_p), P(C.c_int64), C.c_int32, P(Params), C.c_int32, P(C.c_double)]
    L.sd_format_alt_rows.argtypes = [P(C.c_char_p), C.c_int32, C.c_void_p, P(C.c_char_p), C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_void_p),
                                     P(C.c_size_t)]
    L.sd_chunk_table_size.restype = C.c_int64
    L.sd_chunk_table_size.argtypes = [P(C.c_int64), C.c_int32, C.c_int32, C.c_int32]
    L.sd_decompose_chunk_range.argtypes = [P(C.c_char_p), P(C.c_int64), C.c_int32, P(C.c_char_p), P(C.c_int32),
                                           C.c_int32, P(Params), C.c_int64, C.c_int64, P(P(Rec)),
                                           P(P(C.c_int64)), C.c_char_p, C.c_size_t]
    L.sd_assemble_tsv.argtypes = [P(C.c_char_p), P(C.c_int64), C.c_int32, P(C.c_char_p), C.c_int32, P(Params),
                                  C.c_void_p, C.c_void_p, C.c_int64, P(C.c_void_p), P(C.c_size_t),
                                  C.c_char_p, C.c_size_t]
    L.sd_stream_create.argtypes = [P(C.c_void_p), P(Params), P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_int32,
                                   C.c_char_p, C.c_size_t]
    L.sd_stream_destroy.argtypes = [C.c_void_p]
    L.sd_stream_submit.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_int64), C.c_int32, C.c_char_p, C.c_size_t]
    L.sd_stream_collect.argtypes = [C.c_void_p, P(P(Rec)), P(P(C.c_int64)), P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_stream_stats.argtypes = [C.c_void_p, P(C.c_double)]
    L.sd_stream_create_final.argtypes = [P(C.c_void_p), P(Params), P(C.c_char_p), P(C.c_char_p), P(C.c_int32), C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, P(C.c_double), C.c_char_p, C.c_size_t]
    L.sd_stream_collect_final.argtypes = [C.c_void_p, P(P(FinalRec)), P(P(C.c_int64)), P(C.c_int64), P(P(C.c_double)),
                                          C.c_char_p, C.c_size_t]
    L.sd_stream_keys.argtypes = [C.c_void_p, P(C.c_char_p), C.c_int32, P(C.c_int32)]
    L.sd_stream_final_stats.argtypes = [C.c_void_p, P(C.c_double)]
    L.sd_stream_info.argtypes = [C.c_void_p, P(C.c_int64)]
    L.sd_pack_bases.restype = C.c_int32
    L.sd_pack_bases.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.sd_write_records.argtypes = [C.c_char_p, P(Params), P(C.c_char_p), C.c_int32, P(C.c_char_p), C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_read_records.argtypes = [C.c_char_p, P(Records), C.c_char_p, C.c_size_t]
    L.sd_records_free.argtypes = [P(Records)]
    L.sd_records_free.restype = None
    L.sd_records_to_raw_tsv.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t]
    L.sd_decompose_files_records.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_char_p, C.c_char_p, C.c_size_t]
    L.sd_run_files_records.argtypes = [C.c_char_p, C.c_char_p, P(Params), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                       C.c_int32, C.c_int32, P(C.c_double), C.c_char_p, C.c_size_t]
    L.sd_run_files_devices.argtypes = [C.c_char_p, C.c_char_p, P(Params), P(C.c_int32), C.c_int32, C.c_char_p, C.c_char_p,
                                       C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, P(C.c_double), C.c_char_p, C.c_size_t]
    L.sd_last_run_device_stats.argtypes = [P(C.c_int64), P(C.c_double), C.c_int32]
    L.sd_multi_device_selftest.argtypes = [C.c_char_p, C.c_size_t]
    L.sd_stream_create_devices.argtypes = [P(C.c_void_p), P(Params), P(C.c_int32), C.c_int32, P(C.c_char_p), P(C.c_int32),
                                           C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sd_stream_create_final_devices.argtypes = [P(C.c_void_p), P(Params), P(C.c_int32), C.c_int32, P(C.c_char_p),
                                                 P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 P(C.c_double), C.c_char_p, C.c_size_t]
    L.sd_stream_device_stats.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double), C.c_int32]
    L.sd_profile_segments.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_char_p),
                                      P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.sd_profile_segments_dev.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_char_p),
                                          P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.sd_msa_row_offsets.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.sd_msa_row_offsets.restype = C.c_int64
    L.sd_msa_segments.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_char_p),
                                  P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_msa_segments_dev.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_char_p),
                                      P(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
    L.sd_msa_kernel_bench.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_char_p), P(C.c_int32),
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float),
                                      P(C.c_int64)]
    L.sd_msa_tables_create.argtypes = [P(C.c_void_p), C.c_void_p, C.c_int32, P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_char_p,
                                       C.c_size_t]
    L.sd_msa_tables_destroy.argtypes = [C.c_void_p]
    L.sd_msa_tables_destroy.restype = None
    L.sd_msa_final_size_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p, P(C.c_int64), P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_msa_final_write_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_lag_segments.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_lag_segments_dev.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_lag_final_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_lag_final_host.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    L.sd_lag_identities.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.sd_lag_identities.restype = None
    L.sd_lag_periods.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.sd_lag_periods.restype = None
    L.sd_lag_kernel_bench.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float),
                                      P(C.c_int64)]
    L.sd_heat_layout.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, P(C.c_int64), P(C.c_int64)]
    L.sd_heat_segments.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_heat_segments_dev.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_heat_final_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                    C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_heat_final_host.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_heat_identities.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.sd_heat_identities.restype = None
    L.sd_heat_kernel_bench.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                       C.c_int64, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float),
                                       P(C.c_int64)]
    L.sd_autocorr_layout.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, P(C.c_int64)]
    L.sd_autocorr_host.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_autocorr_dev.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_autocorr_reads_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_autocorr_positions.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    L.sd_autocorr_peaks.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.sd_autocorr_seed.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_int64, P(C.c_int64), P(C.c_int64)]
    L.sd_autocorr_info.argtypes = [P(C.c_int64)]
    L.sd_autocorr_info.restype = None
    L.sd_autocorr_kernel_bench.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_int64)]
    L.sd_motif_compile.argtypes = [P(C.c_char_p), P(C.c_char_p), C.c_int32, C.c_int32, P(C.c_int32), C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_motif_host.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                P(C.c_void_p), P(C.c_int64), C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_motif_dev.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                               P(C.c_void_p), P(C.c_int64), C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_motif_reads_size_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_motif_reads_write_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.sd_motif_info.argtypes = [P(C.c_int64)]
    L.sd_motif_info.restype = None
    L.sd_motif_kernel_bench.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int64)]
    L.sd_motif_edit_host.argtypes = L.sd_motif_host.argtypes
    L.sd_motif_edit_dev.argtypes = L.sd_motif_dev.argtypes
    L.sd_motif_edit_reads_size_dev.argtypes = L.sd_motif_reads_size_dev.argtypes
    L.sd_motif_edit_reads_write_dev.argtypes = L.sd_motif_reads_write_dev.argtypes
    L.sd_motif_edit_info.argtypes = [P(C.c_int64)]
    L.sd_motif_edit_info.restype = None
    L.sd_motif_edit_kernel_bench.argtypes = L.sd_motif_kernel_bench.argtypes
    V = C.c_void_p
    cyc = [C.c_char_p, V, V, C.c_int32]   # text, off, lens, n
    L.sd_cyclic_pairs_host.argtypes = cyc + [V, V, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_char_p, C.c_size_t]
    L.sd_cyclic_pairs_dev.argtypes = cyc + [V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_char_p, C.c_size_t]
    L.sd_cyclic_merge_host.argtypes = cyc + [V, C.c_int32, C.c_int32, C.c_int32, V, V, V, V, V, P(C.c_int32), C.c_char_p, C.c_size_t]
    L.sd_cyclic_merge_dev.argtypes = cyc + [V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, V, V, V, V, P(C.c_int32), C.c_char_p, C.c_size_t]
    L.sd_cyclic_canon.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, P(C.c_int64), P(C.c_int32)]
    L.sd_cyclic_info.argtypes = [P(C.c_int64)]
    L.sd_cyclic_info.restype = None
    L.sd_cyclic_kernel_bench.argtypes = cyc + [V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_int64),
                                               V, V, V]
    L.sd_cyclic_pairs_team_host.argtypes = cyc + [V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_char_p, C.c_size_t]
    L.sd_cyclic_long_info.argtypes = [P(C.c_int64)]
    L.sd_cyclic_long_info.restype = None
    L.sd_cyclic_long_kernel_bench.argtypes = cyc + [V, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_float),
                                                    P(C.c_int64), V, V, V]
    L.sd_dotplot_layout.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, P(C.c_int64), P(C.c_int64)]
    L.sd_dotplot_host.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_dotplot_dev.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_dotplot_reads_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p,
                                       C.c_size_t]
    L.sd_dotplot_info.argtypes = [P(C.c_int64)]
    L.sd_dotplot_info.restype = None
    L.sd_dotplot_hash.argtypes = [C.c_uint64]
    L.sd_dotplot_hash.restype = C.c_uint64
    L.sd_dotplot_kernel_bench.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float),
                                          P(C.c_int64)]
    L.sd_split_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_split_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_split_final_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.sd_split_info.argtypes = [P(C.c_int64)]
    L.sd_split_info.restype = None
    L.sd_split_kernel_bench.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_int64)]
    hor_out = [C.c_void_p] * 10 + [C.c_int64, P(C.c_int64), C.c_char_p, C.c_size_t]   # T .. units, cap_units, info, errbuf
    L.sd_hor_rows.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32] + hor_out
    L.sd_hor_final_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32] + hor_out
    L.sd_hor_name.argtypes = [C.c_uint64, C.c_char_p]
    L.sd_hor_info.argtypes = [P(C.c_int64)]
    L.sd_hor_info.restype = None
    L.sd_last_run_profile.argtypes = [P(C.c_int32), P(C.c_int64), P(C.c_int64), C.c_char_p, C.c_void_p]
    L.sd_stream_profile.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_int64), P(C.c_int64), C.c_char_p,
                                    C.c_void_p]
    L.sd_stream_submit_dev.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), P(C.c_int64), C.c_int32, C.c_void_p,
                                       C.c_char_p, C.c_size_t]
    L.sd_engine_load_reads_dev.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int64), P(C.c_int64), C.c_int32, C.c_void_p,
                                           P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_pack_bases_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, P(C.c_int64)]
    L.sd_engine_filter_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64), P(C.c_int32),
                                          C.c_char_p, C.c_size_t]
    L.sd_stream_peek_dev.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int64), C.c_char_p, C.c_size_t]
    L.sd_stream_collect_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, P(C.c_int64),
                                        C.c_char_p, C.c_size_t]
    L.sd_engine_rows_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, P(C.c_int64),
                                     C.c_char_p, C.c_size_t]
    L.sd_seam_merge_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, P(C.c_int64)]
    L.sd_seam_pieces_selftest.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          P(C.c_int64)]
    L.sd_stream_peek_final_dev.argtypes = [C.c_void_p, P(C.c_int32), P(C.c_int64), P(C.c_int32), C.c_char_p, C.c_size_t]
    L.sd_stream_collect_final_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              P(C.c_int64), C.c_char_p, C.c_size_t]
    sel = [P(C.c_char_p), P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, P(C.c_double), C.c_void_p, C.c_void_p,
           C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    out = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64), P(C.c_int64)]
    L.sd_final_select_host.argtypes = sel + out
    L.sd_final_select_dev.argtypes = sel + [C.c_int32, C.c_void_p] + out
    L.sd_stream_profile_dev.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, P(C.c_int64), C.c_char_p,
                                        C.c_size_t]
    L.sd_stream_profile_stats.argtypes = [C.c_void_p, P(C.c_double)]
    prof = [C.c_char_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_char_p), P(C.c_int32), C.c_int32,
            C.c_int32, C.c_int32, C.c_void_p, P(C.c_int64)]
    L.sd_final_profile_dev.argtypes = prof
    L.sd_final_profile_host.argtypes = prof
    V, I64 = C.c_void_p, C.c_int64
    L.sd_text_tables_create.argtypes = [P(V), P(C.c_char_p), C.c_int32, P(C.c_char_p), C.c_int32, C.c_char_p, C.c_size_t]
    L.sd_text_tables_destroy.argtypes = [V]
    L.sd_text_tables_destroy.restype = None
    L.sd_text_final_size_dev.argtypes = [V, V, I64, V, V, C.c_int32, C.c_int32, V, V, V, V, V, P(I64), P(I64), C.c_char_p,
                                         C.c_size_t]
    L.sd_text_final_write_dev.argtypes = [V, V, I64, V, C.c_int32, C.c_int32, V, V, V, V, I64, V, I64, C.c_char_p, C.c_size_t]
    L.sd_text_raw_size_dev.argtypes = [V, V, I64, V, C.c_int32, V, V, V, V, P(I64), C.c_char_p, C.c_size_t]
    L.sd_text_raw_write_dev.argtypes = [V, V, I64, V, C.c_int32, V, V, V, V, I64, C.c_char_p, C.c_size_t]
    L.sd_text_final_host.argtypes = [V, V, I64, V, V, C.c_int32, C.c_int32, P(V), P(I64), P(V), P(I64), V, V, V, V,
                                     C.c_char_p, C.c_size_t]
    L.sd_text_raw_host.argtypes = [V, V, I64, V, C.c_int32, P(V), P(I64), V, V, C.c_char_p, C.c_size_t]
    L.sd_screen_create.argtypes = [P(C.c_char_p), P(C.c_int32), C.c_int32, C.c_int32, P(V), C.c_char_p, C.c_size_t]
    L.sd_screen_destroy.argtypes = [V]
    L.sd_screen_destroy.restype = None
    L.sd_screen_set_general.argtypes = [V, C.c_int32]
    L.sd_screen_kernel.argtypes = [V, P(C.c_int32)]
    L.sd_screen_kernel_ms.argtypes = [V, C.c_int32]
    L.sd_screen_kernel_ms.restype = C.c_double
    L.sd_screen_kernel_bench.argtypes = [V, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), C.c_char_p, C.c_size_t]
    L.sd_run_files_screen.argtypes = [C.c_char_p, C.c_char_p, P(Params), P(C.c_int32), C.c_int32, C.c_char_p, C.c_char_p,
                                      C.c_char_p, C.c_int32, C.c_int32, P(C.c_double), C.c_int32, C.c_char_p, C.c_char_p,
                                      P(I64), C.c_char_p, C.c_size_t]
    L.sd_screen_chunks.argtypes = [V, P(C.c_char_p), P(I64), C.c_int32, C.c_int32, C.c_int32, V, I64, P(I64), C.c_char_p,
                                   C.c_size_t]
    L.sd_screen_chunks_dev.argtypes = [V, V, P(I64), P(I64), C.c_int32, C.c_int32, C.c_int32, V, V, I64, P(I64), C.c_char_p,
                                       C.c_size_t]
    L.sd_screen_chunks_host.argtypes = [P(C.c_char_p), P(C.c_int32), C.c_int32, P(C.c_char_p), P(I64), C.c_int32, C.c_int32,
                                        C.c_int32, V, I64, P(I64), C.c_char_p, C.c_size_t]
    L.sd_screen_regions.argtypes = [V, V, I64, V, C.c_int32, C.c_int32, C.c_int32, C.c_int32, V, I64, P(I64), C.c_char_p,
                                    C.c_size_t]
    _lib = L
    return L


def _b(s):
    if isinstance(s, (memoryview, bytearray)):   # (region_reads' slices)
        return bytes(s)
    return s if isinstance(s, bytes) else s.encode()


def _strs(seq):
    arr = (C.c_char_p * max(len(seq), 1))()
    for i, s in enumerate(seq):
        arr[i] = _b(s)
    return arr


# ---- the call frame of the analyses: what profile, msa, lags, heat, autocorr, motif, dotplot, split and hor share on this side
# of the C-ABI (csrc/sd_job_dev.hpp is the frame on the other side; DESIGN.md, "the Python side of the frame") ----------------
def _err():
    """the buffer an entry writes its refusal into (errbuf, 1024)"""
    return C.create_string_buffer(1024)


def _check(rc, what):
    """an entry without errbuf: the refusal names the entry"""
    if rc != SD_OK:
        raise SdError(rc, what)


def _text_check(rc, err, fallback=""):
    """an entry with errbuf: its text, or `fallback` where it left none"""
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace") or fallback)


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def _int_arg(who, name, v, lo, hi, say=None, bools=False):
    """who: name = v, must be an integer lo .. hi -- refused before any array is made or any device is touched.  say: the
    words behind "must be an integer" where they are not the range checked (", 1 or more" with hi the C type's limit);
    hi=None, no upper limit, needs them."""
    assert hi is not None or say is not None
    if not (_is_int(v) or (bools and isinstance(v, bool))) or v < lo or (hi is not None and v > hi):
        raise SdError(SD_ERR_PARAM, "%s: %s = %r, must be an integer%s" % (who, name, v, " %d .. %d" % (lo, hi) if say is None else say))
    return v


_Segments = namedtuple("_Segments", "lead n G go pt tb arrays")


def _segments(who, text, starts, ends, group_off=None, pair_tmpl=None, templates=None):
    """The arguments of a segment call as ctypes takes them: .lead = (text, its length, starts, ends, n), then (group_off,
    groups) and (templates, their lengths, T, pair_tmpl or NULL) for those given -- the order of every sd_*_segments entry;
    .n segments, .G groups, .go / .pt the int64 group_off / int32 pair_tmpl arrays, .tb the templates as bytes.  who: the
    caller's name for the refusal of lengths that differ; None: no check (the kernel benches).  The result owns the arrays
    behind the addresses: keep it until the call has returned."""
    import numpy as np
    sb = _b(text)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    en = np.ascontiguousarray(ends, dtype=np.int64)
    n = int(st.shape[0])
    lead, G, go, pt, tb = [sb, len(sb), st.ctypes.data, en.ctypes.data, n], None, None, None, None
    if group_off is not None:
        go = np.ascontiguousarray(group_off, dtype=np.int64)
        if who and (en.shape[0] != n or go.ndim != 1 or go.shape[0] < 1):
            raise SdError(SD_ERR_PARAM, "%s: starts and ends differ in length, or group_off is empty" % who)
        G = len(go) - 1
        lead += [go.ctypes.data, G]
    if pair_tmpl is not None:
        pt = np.ascontiguousarray(pair_tmpl, dtype=np.int32)
        if who and (en.shape[0] != n or pt.shape[0] != n):
            raise SdError(SD_ERR_PARAM, "%s: starts, ends and pair_tmpl differ in length" % who)
    if templates is not None:
        tb = [_b(t) for t in templates]
        tl = (C.c_int32 * max(len(tb), 1))(*[len(t) for t in tb])
        lead += [_strs(tb), tl, len(tb), None if pt is None else pt.ctypes.data]
    return _Segments(tuple(lead), n, G, go, pt, tb, (st, en))


def _reads_text(reads):
    """a list of bytes / str -> (text, offsets, lengths): the reads back to back"""
    import numpy as np
    rs = [_b(s) for s in reads]
    rl = np.ascontiguousarray([len(s) for s in rs], dtype=np.int64).reshape(-1)
    ro = np.zeros(len(rs), dtype=np.int64)
    if len(rs) > 1:
        np.cumsum(rl[:-1], out=ro[1:])
    return b"".join(rs), ro, rl


def _text_reads(who, text, read_off, read_lens):
    """reads given as one buffer with offsets and lengths, as the *_text calls take them -> (text, offsets, lengths), every
    read inside the text"""
    import numpy as np
    tb = _b(text)
    ro = np.ascontiguousarray(read_off, dtype=np.int64).reshape(-1)
    rl = np.ascontiguousarray(read_lens, dtype=np.int64).reshape(-1)
    if len(ro) != len(rl) or (len(rl) and (int(ro.min()) < 0 or int(rl.min()) < 0 or int((ro + rl).max()) > len(tb))):
        raise SdError(SD_ERR_PARAM, "%s: offsets and lengths differ in number, or a read lies outside the text" % who)
    return tb, ro, rl


def segment_clamp(start, end, n):
    """A final row's (start, end) in a read of n bases -> (s0, e), the inclusive segment as the selection measured it; an
    empty segment has e = s0 - 1."""
    s0 = min(max(start, 0), n)
    return s0, min(max(end + 1, s0), n) - 1


def _device_frame(dev, stream):
    """(torch, dev, st) of a call on device tensors: dev = a torch device or an ordinal, st = the torch stream of `stream`
    (_torch_stream)"""
    import torch
    if isinstance(dev, int):
        dev = torch.device("cuda", dev)
    return torch, dev, _torch_stream(torch, dev, stream)


def _dptr(t):
    """the device address of a tensor; NULL for None and for a tensor without elements"""
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _bench(fn, lead, ms_names, info_names, reps):
    """fn(*lead, one float [reps] per name of ms_names, info) of a *_kernel_bench entry -> {name: [ms], ..., name: int, ...}"""
    ms = [(C.c_float * reps)() for _ in ms_names]
    info = (C.c_int64 * len(info_names))()
    _check(fn(*lead, *ms, info), fn.__name__)
    out = {k: [float(x) for x in v] for k, v in zip(ms_names, ms)}
    out.update(zip(info_names, (int(x) for x in info)))
    return out


def _info(fn, names, slots=None):
    """fn(info) of a sd_*_info entry -> {name: int}"""
    info = (C.c_int64 * (slots or len(names)))()
    fn(info)
    return dict(zip(names, (int(x) for x in info)))


FLAG_NO_F16, FLAG_FULL_FLOOR, FLAG_NO_EDTHR_COMPACT, FLAG_FILTER_GENERAL, FLAG_NO_STREAM_IDENT, FLAG_PROGRESS = 1, 2, 4, 8, 16, 32
FLAG_TRACE_V1 = 64
FLAG_NO_IDENT_PRUNE = 256   # --second-best: every homopolymer-compressed pair aligned in full (no distance-only pruning)
FLAG_NO_U16 = 128     # narrow layout: fp16 / int16 cells as in rounds 1-5 instead of the biased-u16 format
FLAG_PROFILE = 512    # per-monomer column profiles of the kept rows (run_files(profile=True), Stream(profile=True))
FLAG_DEVICE_ROWS = 1024   # Stream(device_rows=True): the rows are assembled on the device and stay there
FLAG_DEVICE_FINAL = 2048  # Stream(final=True, device_final=True): the final rows are selected on the device and stay there
FLAG_DEVICE_PROFILE = 4096  # Stream(final=True, device_final=True, device_profile=True): their column profiles are folded there too
FLAG_LENIENT = 8192   # files are read leniently (make_params(lenient=True)): lower case folded, IUPAC codes -> N, CRLF


def make_params(scoring=(-1, -1, -1, 1), part_size=5000, overlap=500, ed_thr=-1, threads=1,
                device=0, kernel=KERNEL_AUTO, max_batch_rows=0, pipe_mode=None, flags=0, f16_guard=0, lenient=False):
    """sd_params; pipe_mode (None = the library default, 0 / 1 / 2), flags (FLAG_* bits) and f16_guard (magnitude
    limit of the fills' fp16 range guard, 0 = 2040) are the reserved[] switches of include/sd_hip.h.  lenient=True sets
    FLAG_LENIENT: the calls that open the two files fold lower case, turn IUPAC ambiguity codes into N and drop the CR
    of CRLF line ends (sd_hip.h, "lenient input"); the default reproduces the reference's errors."""
    L = load()
    p = Params()
    L.sd_params_default(C.byref(p))
    p.ins, p.del_, p.mismatch, p.match = [int(x) for x in scoring]
    p.part_size, p.overlap, p.ed_thr = int(part_size), int(overlap), int(ed_thr)
    p.threads, p.device, p.kernel = int(threads), int(device), int(kernel)
    p.max_batch_rows = int(max_batch_rows)
    p.reserved[0] = 0 if pipe_mode is None else int(pipe_mode) + 1
    p.reserved[1] = int(flags) | (FLAG_LENIENT if lenient else 0)
    p.reserved[2] = int(f16_guard)
    return p


def guard_trips():
    """Batches of this process repeated with integer cells because the fp16 range guard tripped (sd_guard_trips)."""
    L = load()
    L.sd_guard_trips.restype = C.c_int64
    return int(L.sd_guard_trips())


NW_ROUTE_KEYS = ("long_calls", "long_pairs", "long_host_pairs", "long_rounds_max", "short_calls", "short_pairs", "declined_calls")


def nw_route_counts():
    """Which route the device identity calls of this process took so far (sd_nw_route_counts): a dict of the cumulative
    counts NW_ROUTE_KEYS.  Host only; all zero before the first device call."""
    L = load()
    v = (C.c_int64 * 8)()
    L.sd_nw_route_counts.restype = None
    L.sd_nw_route_counts(v)
    return {k: int(v[i]) for i, k in enumerate(NW_ROUTE_KEYS)}


def plan_info(mono_seqs, **kw):
    """The layout the fast kernel family would use for this monomer set and scoring (host only, no GPU needed):
    {"family", "cells_per_lane", "cells", "floor_slots", "waves", "range_bound", "min_first_lane_cells", "max_lane_cells",
    "score_factor", "trace_regs" (0 = one-block int32 traceback), "trace_bound", "bperm_scan", "why"} -- family "generic"
    carries the reason in "why"."""
    L = load()
    p = make_params(**kw)
    ms = [_b(s) for s in mono_seqs]
    ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
    v = (C.c_int64 * 8)()
    err = C.create_string_buffer(4096)
    rc = L.sd_plan_info(C.byref(p), _strs(ms), ml, len(ms), v, err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    cells = {0: "int32", 1: "int16", 2: "f16", 9: "u16", 3: "int16/int8-table", 4: "f16/bf8-table", 5: "f16/bf8-codes x waves", 6: "f16/bf8-codes tiled x waves",
             7: "int16/int8-codes x waves", 8: "int16/int8-codes tiled x waves"}
    return {"family": {1: "generic", 2: "fast"}[v[0]], "cells_per_lane": v[1], "cells": cells.get(v[2], "?") if v[0] == 2 else "int32",
            "floor_slots": v[3], "waves": v[4] & 0xff, "range_bound": (v[4] >> 8) & 0xffffffff, "rebase": v[4] >> 40, "min_first_lane_cells": v[5], "max_lane_cells": v[6],
            "score_factor": v[7] & 0xffff, "trace_regs": (v[7] >> 16) & 0xff, "trace_bound": (v[7] >> 24) & 0xffffffff,
            "bperm_scan": bool((v[7] >> 56) & 1), "why": err.value.decode(errors="replace") if v[0] == 1 else ""}


def plan_floor_levels(mono_seqs, **kw):
    """The floor levels of the narrow fills for this monomer set and scoring (host only, no GPU needed; sd_plan_floor_levels):
    {"family", "cells_per_lane", "pair_rule" (the scoring meets the conditions of the levels by symbol pair), "floor_sym"
    [5] (read symbols A C G T N), "floor_pair" [previous][current], "lane_starts" (per template -- the monomers, then their
    reverse complements -- the first cell of each of its lanes), "why"}; family "generic" carries the reason in "why"."""
    L = load()
    p = make_params(**kw)
    ms = [_b(s) for s in mono_seqs]
    ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
    T, cap = 2 * len(ms), 2 * sum(len(s) for s in ms) + 1
    sym, pair = (C.c_int32 * 5)(), (C.c_int32 * 25)()
    off, start = (C.c_int32 * (T + 1))(), (C.c_int32 * cap)()
    v = (C.c_int64 * 4)()
    err = C.create_string_buffer(4096)
    rc = L.sd_plan_floor_levels(C.byref(p), _strs(ms), ml, len(ms), sym, pair, off, start, cap, v, err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    return {"family": {1: "generic", 2: "fast"}[v[0]], "cells_per_lane": v[1], "pair_rule": bool(v[2]),
            "floor_sym": list(sym), "floor_pair": [list(pair[5 * a:5 * a + 5]) for a in range(5)],
            "lane_starts": [list(start[off[j]:off[j + 1]]) for j in range(T)],
            "why": err.value.decode(errors="replace") if v[0] == 1 else ""}


def release_cache():
    """Return the library's cached device buffers to the driver."""
    load().sd_release_cache()


def device_count():
    return load().sd_device_count()


def decompose_files(reads_fa, monomers_fa, raw_tsv_out, **kw):
    """reads.fa + monomers.fa -> raw TSV file (the bytes `dp` would print on stdout)."""
    L = load()
    p = make_params(**kw)
    err = C.create_string_buffer(4096)
    rc = L.sd_decompose_files(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p),
                              os.fsencode(raw_tsv_out), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def run_files(reads_fa, monomers_fa, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity=0, second_best=False,
              lr_coef=(-31.48494996, 0.41784018, 0.69186882), records_out=None, devices=None, profile=False, screen=None,
              screen_tsv_out=None, **kw):
    """The whole CLI job natively (sd_run_files): raw, final and _alt TSV files from the two FASTA files; with
    records_out also the binary record stream of the raw rows (sd_run_files_records).  devices (a list of ordinals,
    repeats allowed): one pipeline per entry in this process (sd_run_files_devices; `device` is then ignored), the
    same output bytes.  profile=True (SD_FLAG_PROFILE): also the column profiles of the monomers over the rows of the
    final TSV, returned as a formats.Profile (and by last_run_profile()); the three files are unchanged.
    screen=THR (sd_run_files_screen): only the regions of the reads whose chunks come within infix edit distance THR of a
    monomer are decomposed -- per region the rows of the plain job on its substring, positions in the parent read;
    screen_tsv_out: the region file (formats.read_screen).  last_run_screen() gives the job's counts."""
    L = load()
    if profile:
        kw["flags"] = int(kw.get("flags", 0)) | FLAG_PROFILE
    p = make_params(**kw)
    err = C.create_string_buffer(4096)
    coef = (C.c_double * 3)(*[float(x) for x in lr_coef])
    if screen is not None:
        devs = None if devices is None else [int(d) for d in devices]
        arr = None if devs is None else (C.c_int32 * max(len(devs), 1))(*devs)
        counts = (C.c_int64 * 4)()
        rc = L.sd_run_files_screen(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), arr, 0 if devs is None else len(devs),
                                   os.fsencode(raw_tsv_out), os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out),
                                   int(min_identity), 1 if second_best else 0, coef, int(screen),
                                   None if screen_tsv_out is None else os.fsencode(screen_tsv_out),
                                   None if records_out is None else os.fsencode(records_out), counts, err, 4096)
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        global _last_screen
        _last_screen = {"reads": counts[0], "reads_with_region": counts[1], "bases_read": counts[2], "bases_decomposed": counts[3]}
        return last_run_profile() if profile else None
    if devices is not None:
        devs = [int(d) for d in devices]
        arr = (C.c_int32 * max(len(devs), 1))(*devs)
        rc = L.sd_run_files_devices(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), arr, len(devs),
                                    os.fsencode(raw_tsv_out), os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out),
                                    None if records_out is None else os.fsencode(records_out), int(min_identity),
                                    1 if second_best else 0, coef, err, 4096)
    elif records_out is None:
        rc = L.sd_run_files(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), os.fsencode(raw_tsv_out),
                            os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out), int(min_identity), 1 if second_best else 0,
                            coef, err, 4096)
    else:
        rc = L.sd_run_files_records(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), os.fsencode(raw_tsv_out),
                                    os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out), os.fsencode(records_out),
                                    int(min_identity), 1 if second_best else 0, coef, err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    return last_run_profile() if profile else None


_last_screen = None


def last_run_input_stats():
    """What the file indexes of the last file job of this process met (sd_last_run_input_stats), summed over reads and
    monomers: lower (lower-case bases folded), ambiguity (codes turned into N), cr (CRs dropped), copied (records that
    got a buffer of their own because the rule changed them), fastq (FASTQ records), lenient (was the mode on)."""
    v = (C.c_int64 * 8)()
    load().sd_last_run_input_stats(v)
    return {"lower": v[0], "ambiguity": v[1], "cr": v[2], "copied": v[3], "fastq": v[4], "lenient": bool(v[5])}


def last_run_screen():
    """Counts of the last run_files(screen=...) of this process: reads, reads_with_region, bases_read, bases_decomposed."""
    return _last_screen


def _profile_from(fn, *lead, numpy=True):
    """A formats.Profile from the two-call form of sd_last_run_profile / sd_stream_profile (fn(*lead, outputs...))."""
    from . import formats
    n, nc, tb = C.c_int32(), C.c_int64(), C.c_int64()
    rc = fn(*lead, C.byref(n), C.byref(nc), C.byref(tb), None, None)
    if rc != SD_OK:
        raise SdError(rc, "no profile: the call was made without the profile flag")
    text = C.create_string_buffer(max(int(tb.value), 1))
    counts = (C.c_uint64 * max(int(nc.value), 1))()
    rc = fn(*lead, C.byref(n), C.byref(nc), C.byref(tb), text, counts)
    if rc != SD_OK:
        raise SdError(rc, "profile")
    lines = text.value.decode().split("\n")[:n.value]
    names = [x.split("\t")[0] for x in lines]
    seqs = [x.split("\t")[1] for x in lines]
    return formats.profile_from_counts(names, seqs, counts[:int(nc.value)], numpy=numpy)


def last_run_profile(numpy=True):
    """The formats.Profile of the last run_files call of this process made with profile=True (sd_last_run_profile);
    numpy=False gives the counters as lists of row lists (no numpy import: what the command line writes from)."""
    L = load()
    return _profile_from(L.sd_last_run_profile, numpy=numpy)


def profile_segments(seq, starts, ends, templates, pair_tmpl, threads=1, device=None):
    """Column profiles (sd_profile_segments[_dev]) of segments seq[starts[s] .. ends[s]] (inclusive) aligned to
    monomer pair_tmpl[s] >> 1, against its reverse complement when pair_tmpl[s] & 1; templates = the FORWARD monomers.
    Returns the counters: a list over monomers of int64 arrays [L + 1, 12] (formats.PROFILE_COLUMNS).  device=None: host
    threads; device=<ordinal>: the HIP kernel, with the host form for the pairs it does not take."""
    import numpy as np
    from . import formats
    L = load()
    seg = _segments("profile_segments", seq, starts, ends, pair_tmpl=pair_tmpl, templates=templates)
    counts = np.zeros(sum(len(t) + 1 for t in seg.tb) * formats.PROFILE_NCOLS, dtype=np.uint64)
    if device is None:
        rc = L.sd_profile_segments(*seg.lead, int(threads), counts.ctypes.data)
    else:
        rc = L.sd_profile_segments_dev(*seg.lead, int(device), int(threads), counts.ctypes.data)
    _check(rc, "sd_profile_segments" + ("" if device is None else "_dev"))
    return formats.split_counts([len(t) for t in seg.tb], counts.astype(np.int64))


def msa_row_offsets(tlen, pair_tmpl):
    """sd_msa_row_offsets: where the row of each pair begins (n + 1 offsets; the last is the total bytes); tlen = the
    lengths of the FORWARD monomers, pair_tmpl interleaved."""
    import numpy as np
    L = load()
    tl = np.ascontiguousarray(tlen, dtype=np.int32)
    pt = np.ascontiguousarray(pair_tmpl, dtype=np.int32)
    at = np.zeros(len(pt) + 1, dtype=np.int64)
    rc = L.sd_msa_row_offsets(tl.ctypes.data, len(tl), pt.ctypes.data, len(pt), at.ctypes.data)
    if rc < 0:
        raise SdError(int(-rc), "sd_msa_row_offsets")
    return at


def msa_segments(seq, starts, ends, templates, pair_tmpl, threads=1, device=None):
    """One row per pair (sd_msa_segments[_dev]; include/sd_hip.h: SD_MSA_PITCH), the arguments of profile_segments:
    segment seq[starts[s] .. ends[s]] against monomer pair_tmpl[s] >> 1, its reverse complement when pair_tmpl[s] & 1 ->
    formats.Msa(rows, row_at, status, tlen).  device=None: host threads; device=<ordinal>: the HIP kernel, with the
    host form for the pairs it does not take -- the same bytes."""
    import numpy as np
    from . import formats
    L = load()
    seg = _segments("msa_segments", seq, starts, ends, pair_tmpl=pair_tmpl, templates=templates)
    n, pt, T = seg.n, seg.pt, len(seg.tb)
    if n and (T < 1 or int(pt.min()) < 0 or int(pt.max()) >= 2 * T):
        raise SdError(SD_ERR_PARAM, "msa_segments: pair_tmpl outside the %d interleaved templates" % (2 * T))
    lens = [len(t) for t in seg.tb]
    total = sum(formats.msa_pitch(lens[int(p) >> 1]) for p in pt.tolist())
    rows = np.zeros(max(total, 1), dtype=np.uint8)
    row_at = np.zeros(n + 1, dtype=np.int64)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    if device is None:
        rc = L.sd_msa_segments(*seg.lead, int(threads), rows.ctypes.data, row_at.ctypes.data, status.ctypes.data)
    else:
        rc = L.sd_msa_segments_dev(*seg.lead, int(device), int(threads), rows.ctypes.data, row_at.ctypes.data, status.ctypes.data)
    _check(rc, "sd_msa_segments" + ("" if device is None else "_dev"))
    return formats.Msa(rows[:total], row_at, status[:n], lens)


def msa_kernel_bench(seq, starts, ends, templates, pair_tmpl, device=0, warmup=2, reps=5):
    """sd_msa_kernel_bench: the row kernel and the profile kernel timed in turn on the same pairs (HIP events) ->
    {"msa_ms": [...], "profile_ms": [...], "K", "grid", "items", "pairs", "msa_lds_bytes", "staged", "profile_lds_bytes",
    "ck_slots"}."""
    seg = _segments(None, seq, starts, ends, pair_tmpl=pair_tmpl, templates=templates)
    return _bench(load().sd_msa_kernel_bench, seg.lead + (int(device), int(warmup), int(reps)), ("msa_ms", "profile_ms"),
                  ("K", "grid", "items", "pairs", "msa_lds_bytes", "staged", "profile_lds_bytes", "ck_slots"), reps)


def _msa_key_table(keys, mono_names):
    """key -> interleaved template, by name; a repeated monomer name is refused: a row's key must name one template."""
    il = {}
    for m, n in enumerate(mono_names):
        n = n if isinstance(n, str) else n.decode()
        for x, name in ((2 * m, n), (2 * m + 1, n + "'")):
            if name in il:
                raise SdError(SD_ERR_PARAM, "monomer name %s is not unique: a row's key must name one template" % name)
            il[name] = x
    try:
        return [il[k if isinstance(k, str) else k.decode()] for k in keys]
    except KeyError as e:
        raise SdError(SD_ERR_PARAM, "key %s names no monomer" % e)


def final_msa_host(final_rows, read_seqs, keys, mono_names, mono_seqs, threads=1):
    """The rows (formats.Msa) of the kept rows of a final-mode job -- a FinalRows or its (rows, row_off, alt) -- without
    a device: row i's segment read[start : end + 1], clamped as the selection measured it, against its own template
    keys[best].  read_seqs: the job's reads in submit order; keys: Stream.keys().  -> (Msa, pair_tmpl); every status is
    0 or 1."""
    import numpy as np
    kil = _msa_key_table(keys, mono_names)
    rows = final_rows[0]
    text, off, lens = _reads_text(read_seqs)
    off, lens = off.tolist(), lens.tolist()
    st, en, pt = [], [], []
    for read, start, end, best in zip(rows["read"].tolist(), rows["start"].tolist(), rows["end"].tolist(), rows["best"].tolist()):
        s0, e = segment_clamp(start, end, lens[read])
        st.append(off[read] + s0)
        en.append(off[read] + e)
        pt.append(kil[best])
    if not text:
        text, st, en = b"N", [0] * len(st), [-1] * len(en)
    return msa_segments(text, st, en, mono_seqs, pt, threads=threads), np.asarray(pt, dtype=np.int32)


class DeviceMsa(namedtuple("DeviceMsa", "rows row_at status tlen classes")):
    """The rows of --msa in device memory (final_msa_device): rows = a flat uint8 torch tensor, row_at = int64 [n + 1],
    status = uint8 [n] (0 no instance, 1 computed, 2 left out: a pair the row kernel does not take), all on the final rows'
    device; tlen = the forward monomers' lengths and classes = (status-0 rows, kernel pairs, pairs left out) on the host."""
    __slots__ = ()

    def to_host(self):
        """-> formats.Msa"""
        from . import formats
        return formats.Msa(self.rows.cpu().numpy(), self.row_at.cpu().numpy(), self.status.cpu().numpy(), list(self.tlen))


class MsaTables:
    """What final_msa_device needs of a monomer set (sd_msa_tables): key -> interleaved template and the forward monomers,
    uploaded by the first call that uses them and reused by later ones; close() waits for the last of those calls'
    kernels.  A repeated monomer name is refused: a row's key must name one template."""

    def __init__(self, keys, mono_names, mono_seqs):
        import numpy as np
        self.L = load()
        kil = np.ascontiguousarray(_msa_key_table(keys, mono_names), dtype=np.int32)
        ms = [_b(s) for s in mono_seqs]
        self.tlen = [len(s) for s in ms]
        self.n_keys = len(kil)
        self.h = C.c_void_p()
        err = _err()
        _text_check(self.L.sd_msa_tables_create(C.byref(self.h), kil.ctypes.data, len(kil), _strs(ms),
                                                (C.c_int32 * max(len(ms), 1))(*self.tlen), len(ms), err, 1024), err)

    def close(self):
        if self.h:
            self.L.sd_msa_tables_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def final_msa_device(dfr, reads, keys, mono_names, mono_seqs, stream=None, tables=None, cap=None):
    """The rows of --msa of a DeviceFinalRows, computed on its device from the reads it was selected from (sd_msa_final_size_dev
    / sd_msa_final_write_dev) -> DeviceMsa.  reads: the DeviceReads that was submitted; keys: Stream.keys(); tables: an
    MsaTables over the same set, to upload it once for many jobs.  torch allocates the outputs on `stream` (the
    convention of format_final_device) and the library fills them there: the host waits for the size and the class
    counts only.  Pairs the row kernel does not take keep status 2 and an empty row (final_msa_host computes them).
    cap: the bytes to allocate for the rows (default: what the size pass asks for)."""
    import torch
    L = load()
    dev = dfr.row_off.device
    st = _torch_stream(torch, dev, stream)
    n = int(dfr.n_rows)
    if dfr.row_off.shape[0] != reads.n + 1:
        raise SdError(SD_ERR_PARAM, "final_msa_device: %d reads for the rows of %d" % (reads.n, dfr.row_off.shape[0] - 1))
    t = tables if tables is not None else MsaTables(keys, mono_names, mono_seqs)
    err = C.create_string_buffer(1024)
    ptr = lambda x: C.c_void_p(x.data_ptr() if x.numel() else 0)   # noqa: E731
    try:
        if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
            ev = torch.cuda.Event()
            ev.record(_torch_stream(torch, dev, reads.stream))
            st.wait_event(ev)
        with torch.cuda.stream(st):
            row_at = torch.empty(n + 1, dtype=torch.int64, device=dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)
        total, cls = C.c_int64(), (C.c_int64 * 3)()
        _text_check(L.sd_msa_final_size_dev(t.h, ptr(dfr.rows), n, C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n,
                                            dev.index or 0, C.c_void_p(st.cuda_stream), ptr(row_at), C.byref(total), cls, err, 1024),
                    err)
        nbytes = total.value if cap is None else int(cap)
        with torch.cuda.stream(st):
            rows = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _text_check(L.sd_msa_final_write_dev(t.h, ptr(dfr.rows), n, dev.index or 0, C.c_void_p(st.cuda_stream), ptr(row_at),
                                             ptr(rows), nbytes, ptr(status), err, 1024), err)
    finally:
        if tables is None:
            t.close()
    return DeviceMsa(rows, row_at, status, t.tlen, tuple(int(x) for x in cls))


def final_msa_classes(final_rows, read_lens, keys, mono_names, mono_seqs):
    """The host's plan of final_msa_device: (rows that are no instance, pairs of the row kernel, pairs it leaves out) by
    the rule of csrc/sd_final_prof_dev.hpp, and the per-row class (0 / 1 / 2) as a list."""
    kil = _msa_key_table(keys, mono_names)
    tl = [len(_b(s)) for s in mono_seqs]
    tmax = max(tl)
    rows = final_rows[0]
    out = []
    for read, start, end, best in zip(rows["read"].tolist(), rows["start"].tolist(), rows["end"].tolist(), rows["best"].tolist()):
        s0, e = segment_clamp(start, end, int(read_lens[read]))
        q = e + 1 - s0
        t = tl[kil[best] >> 1]
        if q <= 0 or t <= 0:
            out.append(0)
        elif tmax <= 512 and q <= 1024 and not 20 * ((q + 63) // 64) * t + 8 * t >= 1024 * 1024:
            out.append(1)
        else:
            out.append(2)
    return (out.count(0), out.count(1), out.count(2)), out


LAG_DMAX = 255


def _lag_d(D, who):
    """1 <= D <= 255, refused here before any array is made or any device is touched"""
    return _int_arg(who, "D", D, 1, LAG_DMAX)


def lag_segments(text, starts, ends, group_off, D, device=None, threads=1):
    """Identity of every segment to its next D neighbours in the same group (sd_lag_segments[_dev]; include/sd_hip.h):
    segment s = text[starts[s] .. ends[s]] (inclusive), segments group_off[g] .. group_off[g + 1] are the rows of one read,
    pair (s, d) aligns segment s as the query against segment s + d as the target -> formats.Lags(dist, matches, sums) with
    dist / matches int32 [n, D] (-1 / 0: no partner) and sums int64 [groups, D, 3] = (pairs, sum of matches, sum of dist +
    matches).  device=None: host threads; device=<ordinal>: the lane kernel, with the host form for the pairs it does not
    take -- the same bytes."""
    import numpy as np
    from . import formats
    D = _lag_d(D, "lag_segments")
    L = load()
    seg = _segments("lag_segments", text, starts, ends, group_off=group_off)
    dist = np.zeros((seg.n, D), dtype=np.int32)
    matches = np.zeros((seg.n, D), dtype=np.int32)
    sums = np.zeros((seg.G, D, 3), dtype=np.int64)
    if device is None:
        rc = L.sd_lag_segments(*seg.lead, D, int(threads), dist.ctypes.data, matches.ctypes.data, sums.ctypes.data)
    else:
        rc = L.sd_lag_segments_dev(*seg.lead, D, int(device), int(threads), dist.ctypes.data, matches.ctypes.data, sums.ctypes.data)
    _check(rc, "sd_lag_segments" + ("" if device is None else "_dev"))
    return formats.Lags(dist, matches, sums)


def lag_identities(dist, matches):
    """float64 identities in percent of (dist, matches), -1 where dist < 0: the identity column's arithmetic
    (sd_lag_identities)"""
    import numpy as np
    d = np.ascontiguousarray(dist, dtype=np.int32)
    m = np.ascontiguousarray(matches, dtype=np.int32)
    out = np.zeros(d.shape, dtype=np.float64)
    load().sd_lag_identities(d.ctypes.data, m.ctypes.data, d.size, out.ctypes.data)
    return out


def lag_periods(sums):
    """(period int32 [groups], pooled identity float64 [groups, D]) of sums [groups, D, 3] by the library's rule
    (sd_lag_periods; csrc/sd_lags.hpp).  formats.lag_period is the same rule in Python integers."""
    import numpy as np
    s = np.ascontiguousarray(sums, dtype=np.int64)
    G, D = int(s.shape[0]), int(s.shape[1])
    period = np.zeros(G, dtype=np.int32)
    pooled = np.zeros((G, D), dtype=np.float64)
    load().sd_lag_periods(s.ctypes.data, G, D, period.ctypes.data, pooled.ctypes.data)
    return period, pooled


def lag_kernel_bench(text, starts, ends, group_off, D, device=0, warmup=2, reps=5):
    """sd_lag_kernel_bench -> {"group_ms", "pairs_ms", "walk_ms", "ident_ms": [...], "pairs", "host_pairs", "K", "K_pairs",
    "ident_ck_slots", "ident_grid", "grid", "ck_slots"}."""
    D = _lag_d(D, "lag_kernel_bench")
    seg = _segments(None, text, starts, ends, group_off=group_off)
    return _bench(load().sd_lag_kernel_bench, seg.lead + (D, int(device), int(warmup), int(reps)),
                  ("group_ms", "pairs_ms", "walk_ms", "ident_ms"),
                  ("pairs", "host_pairs", "K", "K_pairs", "ident_ck_slots", "ident_grid", "grid", "ck_slots"), reps)


class DeviceLags(namedtuple("DeviceLags", "dist matches sums classes")):
    """The lag identities of a DeviceFinalRows in device memory (final_lags_device): dist / matches = int32 [n_rows, D] torch
    tensors, sums = int64 [n_reads, D, 3], on the rows' device; classes = (entries with dist -1, pairs of the lane kernel,
    pairs left out as -2) on the host."""
    __slots__ = ()

    def to_host(self):
        """-> formats.Lags"""
        from . import formats
        return formats.Lags(self.dist.cpu().numpy(), self.matches.cpu().numpy(), self.sums.cpu().numpy())


def final_lags_device(dfr, reads, D, stream=None):
    """Identity of every final row to its next D neighbours in the same read, computed on the rows' device from the reads
    they were selected from (sd_lag_final_dev) -> DeviceLags.  dfr: a DeviceFinalRows; reads: the DeviceReads that was
    submitted.  torch allocates the outputs on `stream` and the library fills them there; the host waits once, for the
    class counts.  Pairs the lane kernel does not take keep dist -2 (final_lags_host computes them)."""
    D = _lag_d(D, "final_lags_device")
    import torch
    L = load()
    dev = dfr.row_off.device
    st = _torch_stream(torch, dev, stream)
    n = int(dfr.n_rows)
    if dfr.row_off.shape[0] != reads.n + 1:
        raise SdError(SD_ERR_PARAM, "final_lags_device: %d reads for the rows of %d" % (reads.n, dfr.row_off.shape[0] - 1))
    err = C.create_string_buffer(1024)
    ptr = lambda x: C.c_void_p(x.data_ptr() if x.numel() else 0)   # noqa: E731
    if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
        ev = torch.cuda.Event()
        ev.record(_torch_stream(torch, dev, reads.stream))
        st.wait_event(ev)
    with torch.cuda.stream(st):
        dist = torch.empty((n, D), dtype=torch.int32, device=dev)
        matches = torch.empty((n, D), dtype=torch.int32, device=dev)
        sums = torch.empty((reads.n, D, 3), dtype=torch.int64, device=dev)
    cls = (C.c_int64 * 3)()
    _text_check(L.sd_lag_final_dev(ptr(dfr.rows), n, C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n, D, dev.index or 0,
                                   C.c_void_p(st.cuda_stream), ptr(dist), ptr(matches), ptr(sums), cls, err, 1024), err)
    return DeviceLags(dist, matches, sums, tuple(int(x) for x in cls))


def final_lags_host(final_rows, read_seqs, D, threads=1):
    """final_lags_device without a device (sd_lag_final_host): final_rows = a FinalRows or its (rows, row_off, alt),
    read_seqs = the job's reads in submit order -> formats.Lags; every pair is computed."""
    import numpy as np
    from . import formats
    D = _lag_d(D, "final_lags_host")
    L = load()
    rows = np.ascontiguousarray(final_rows[0])
    text, ro, rl = _reads_text(read_seqs)
    n, R = int(rows.shape[0]), len(rl)
    dist = np.zeros((n, D), dtype=np.int32)
    matches = np.zeros((n, D), dtype=np.int32)
    sums = np.zeros((R, D, 3), dtype=np.int64)
    _check(L.sd_lag_final_host(rows.ctypes.data, n, text or b"N", ro.ctypes.data, rl.ctypes.data, R, D, int(threads),
                               dist.ctypes.data, matches.ctypes.data, sums.ctypes.data), "sd_lag_final_host")
    return formats.Lags(dist, matches, sums)


HEAT_CELLS_MAX = 1 << 25
HEAT_BMAX = 1 << 20


def _heat_args(B, W, max_pairs, who):
    """1 <= B <= 2^20, W >= 0, max_pairs >= 0, refused here before any array is made or any device is touched"""
    return (_int_arg(who, "B", B, 1, HEAT_BMAX), _int_arg(who, "W", W, 0, (1 << 62) - 1, ", 0 (no limit) or more"),
            _int_arg(who, "max_pairs", max_pairs, 0, (1 << 62) - 1, ", 0 (no limit) or more"))


def heat_layout(group_off, B, W=0):
    """The closed forms of the heatmap (sd_heat_layout; include/sd_hip.h): for groups of group_off[g + 1] - group_off[g] rows,
    B rows per bin and pairs up to W rows apart (0: no limit) -> (cell_off int64 [groups + 1], nb int64 [groups], cells, pairs).
    No device is touched, nothing is refused for size."""
    import numpy as np
    B, W, _ = _heat_args(B, W, 0, "heat_layout")
    go = np.ascontiguousarray(group_off, dtype=np.int64)
    if go.ndim != 1 or go.shape[0] < 1:
        raise SdError(SD_ERR_PARAM, "heat_layout: group_off is empty")
    G = int(go.shape[0]) - 1
    cell_off = np.zeros(G + 1, dtype=np.int64)
    cells, pairs = C.c_int64(0), C.c_int64(0)
    _check(load().sd_heat_layout(go.ctypes.data, G, B, W, cell_off.ctypes.data, C.byref(cells), C.byref(pairs)), "sd_heat_layout")
    nb = (np.diff(go) + B - 1) // B
    return cell_off, nb.astype(np.int64), int(cells.value), int(pairs.value)


def heat_segments(text, starts, ends, group_off, B, W=0, device=None, threads=1, max_pairs=0, which=0):
    """All-against-all identity of the segments of each group, as sums per bin (sd_heat_segments[_dev]; include/sd_hip.h):
    segments and groups as lag_segments takes them, B rows per bin, pairs (x, y), x < y, up to W rows apart (0: no limit);
    query = the earlier segment -> formats.Heat(sums, cell_off, nb, B, W), sums int64 [cells, 3] = (pairs, sum of matches, sum
    of dist + matches) per cell of each group's upper triangle.  device=None: host threads (which=1: only the pairs the
    kernel would leave to the host); device=<ordinal>: the kernel plus the host form for the pairs it does not take -- the
    same bytes; the Heat then carries .classes = (kernel pairs, host pairs, pairs with an empty side).  More than
    HEAT_CELLS_MAX cells, or more than max_pairs pairs (0: no limit), are refused before any alignment."""
    import numpy as np
    from . import formats
    B, W, max_pairs = _heat_args(B, W, max_pairs, "heat_segments")
    L = load()
    seg = _segments("heat_segments", text, starts, ends, group_off=group_off)
    go, G = seg.go, seg.G
    err = _err()
    # the sums are sized by the closed forms; a layout the library would refuse gets one cell, and the library's refusal
    cell_off = np.zeros(G + 1, dtype=np.int64)
    cells, pairs = C.c_int64(0), C.c_int64(0)
    ok = bool((np.diff(go) >= 0).all()) and L.sd_heat_layout(go.ctypes.data, G, B, W, cell_off.ctypes.data, C.byref(cells), C.byref(pairs)) == SD_OK
    n_cells = int(cells.value) if ok and cells.value <= HEAT_CELLS_MAX and (max_pairs == 0 or pairs.value <= max_pairs) else 0
    sums = np.zeros((max(n_cells, 1), 3), dtype=np.int64)
    cls = (C.c_int64 * 3)()
    if device is None:
        rc = L.sd_heat_segments(*seg.lead, B, W, max_pairs, int(which), int(threads), sums.ctypes.data, err, 1024)
    else:
        rc = L.sd_heat_segments_dev(*seg.lead, B, W, max_pairs, int(device), int(threads), sums.ctypes.data, cls, err, 1024)
    _text_check(rc, err)
    heat = formats.Heat(sums[:n_cells], cell_off, (np.diff(go) + B - 1) // B, B, W)
    heat.classes = tuple(int(x) for x in cls) if device is not None else None
    return heat


def heat_identities(sums):
    """float64 pooled identities in percent of sums [cells, 3], -1 for a cell without pairs (sd_heat_identities)"""
    import numpy as np
    s = np.ascontiguousarray(sums, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(s.shape[0], dtype=np.float64)
    load().sd_heat_identities(s.ctypes.data, s.shape[0], out.ctypes.data)
    return out


def heat_kernel_bench(text, starts, ends, group_off, B, W=0, device=0, warmup=2, reps=5):
    """sd_heat_kernel_bench -> {"group_ms", "pairs_ms", "walk_ms": [...], "pairs", "host_pairs", "K", "items", "cells", "K_items",
    "grid", "ck_slots"}."""
    B, W, _ = _heat_args(B, W, 0, "heat_kernel_bench")
    seg = _segments(None, text, starts, ends, group_off=group_off)
    return _bench(load().sd_heat_kernel_bench, seg.lead + (B, W, int(device), int(warmup), int(reps)), ("group_ms", "pairs_ms", "walk_ms"),
                  ("pairs", "host_pairs", "K", "items", "cells", "K_items", "grid", "ck_slots"), reps)


class DeviceHeat(namedtuple("DeviceHeat", "sums cell_off nb classes")):
    """The heatmap sums of a DeviceFinalRows in device memory (final_heat_device): sums = int64 [cells, 3], cell_off = int64
    [n_reads + 1], nb = int64 [n_reads] torch tensors on the rows' device; classes = (pairs of the kernel, pairs left out for
    the host, pairs with an empty side) on the host."""
    __slots__ = ()

    def to_host(self, B, W=0):
        """-> formats.Heat"""
        from . import formats
        return formats.Heat(self.sums.cpu().numpy(), self.cell_off.cpu().numpy(), self.nb.cpu().numpy(), B, W)


def final_heat_device(dfr, reads, B, W=0, stream=None, max_pairs=0):
    """All-against-all identity of the final rows of each read, as sums per bin, computed on the rows' device from the reads
    they were selected from (sd_heat_final_dev) -> DeviceHeat.  dfr: a DeviceFinalRows; reads: the DeviceReads that was
    submitted.  The cells come from the rows per read (dfr.row_off, read once); torch allocates the outputs on `stream` and
    the library fills them there.  Pairs the kernel does not take are left out and counted in classes[1]
    (final_heat_host(which=1) computes them)."""
    B, W, max_pairs = _heat_args(B, W, max_pairs, "final_heat_device")
    import numpy as np
    import torch
    L = load()
    dev = dfr.row_off.device
    st = _torch_stream(torch, dev, stream)
    n = int(dfr.n_rows)
    if dfr.row_off.shape[0] != reads.n + 1:
        raise SdError(SD_ERR_PARAM, "final_heat_device: %d reads for the rows of %d" % (reads.n, dfr.row_off.shape[0] - 1))
    cell_off, nb, cells, pairs = heat_layout(dfr.row_off.cpu().numpy(), B, W)
    if cells > HEAT_CELLS_MAX:
        raise SdError(SD_ERR_PARAM, "final_heat_device: %d cells, the cap is %d (HEAT_CELLS_MAX): use more rows per bin" % (cells, HEAT_CELLS_MAX))
    err = C.create_string_buffer(1024)
    ptr = lambda x: C.c_void_p(x.data_ptr() if x.numel() else 0)   # noqa: E731
    if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
        ev = torch.cuda.Event()
        ev.record(_torch_stream(torch, dev, reads.stream))
        st.wait_event(ev)
    with torch.cuda.stream(st):
        sums = torch.empty((cells, 3), dtype=torch.int64, device=dev)
        d_off = torch.from_numpy(cell_off).to(dev, non_blocking=False)
        d_nb = torch.from_numpy(np.ascontiguousarray(nb)).to(dev, non_blocking=False)
    cls = (C.c_int64 * 3)()
    _text_check(L.sd_heat_final_dev(ptr(dfr.rows), n, C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n, B, W, max_pairs,
                                    dev.index or 0, C.c_void_p(st.cuda_stream), ptr(sums), cells, cls, err, 1024), err)
    return DeviceHeat(sums, d_off, d_nb, tuple(int(x) for x in cls))


def final_heat_host(final_rows, read_seqs, B, W=0, threads=1, max_pairs=0, which=0):
    """final_heat_device without a device (sd_heat_final_host): final_rows = a FinalRows or its (rows, row_off, alt),
    read_seqs = the job's reads in submit order -> formats.Heat with .classes; which=0: every pair, which=1: only the pairs
    the kernel leaves out."""
    import numpy as np
    from . import formats
    B, W, max_pairs = _heat_args(B, W, max_pairs, "final_heat_host")
    L = load()
    rows = np.ascontiguousarray(final_rows[0])
    text, ro, rl = _reads_text(read_seqs)
    n, R = int(rows.shape[0]), len(rl)
    counts = np.bincount(rows["read"], minlength=R) if n else np.zeros(R, dtype=np.int64)
    if counts.shape[0] != R:
        raise SdError(SD_ERR_PARAM, "final_heat_host: a row's read index lies outside the %d reads" % R)
    go = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cell_off, nb, cells, pairs = heat_layout(go, B, W)
    n_cells = cells if cells <= HEAT_CELLS_MAX else 0   # (over the cap: the library refuses before it writes)
    sums = np.zeros((max(n_cells, 1), 3), dtype=np.int64)
    cls = (C.c_int64 * 3)()
    err = _err()
    _text_check(L.sd_heat_final_host(rows.ctypes.data, n, text or b"N", ro.ctypes.data, rl.ctypes.data, R, B, W, max_pairs,
                                     int(which), int(threads), sums.ctypes.data, n_cells, cls, err, 1024), err)
    heat = formats.Heat(sums[:n_cells], cell_off, nb, B, W)
    heat.classes = tuple(int(x) for x in cls)
    return heat


AUTOCORR_KMAX = 32
AUTOCORR_DMAX = 1 << 20
AUTOCORR_CELLS_MAX = 1 << 27


def _autocorr_args(k, D, W, who):
    """1 <= k <= 32, 1 <= D <= 2^20, W >= 0, refused here before any array is made or any device is touched"""
    return (_int_arg(who, "k", k, 1, AUTOCORR_KMAX), _int_arg(who, "D", D, 1, AUTOCORR_DMAX),
            _int_arg(who, "window", W, 0, (1 << 62) - 1, ", 0 (one window) or more"))


def autocorr_info():
    """sd_autocorr_info -> {"tile": bases of a workgroup's tile, "lags": lags of a workgroup, "launch_work": the most
    base-lag products of one launch of the pair kernel, "launches": its launches in this process so far}"""
    return _info(load().sd_autocorr_info, ("tile", "lags", "launch_work", "launches"))


def autocorr_layout(read_lens, window=0):
    """The windows of reads of the given lengths (sd_autocorr_layout) -> (win_off int64 [n + 1], win_start, win_end int64
    [windows], windows): read r owns the windows win_off[r] .. win_off[r + 1], each [win_start, win_end) in its read."""
    import numpy as np
    _, _, W = _autocorr_args(1, 1, window, "autocorr_layout")
    rl = np.ascontiguousarray(read_lens, dtype=np.int64).reshape(-1)
    win_off = np.zeros(len(rl) + 1, dtype=np.int64)
    total = C.c_int64(0)
    _check(load().sd_autocorr_layout(rl.ctypes.data, len(rl), W, win_off.ctypes.data, C.byref(total)),
           "sd_autocorr_layout: a negative read length, or 2^62 windows or more")
    nw = np.diff(win_off)
    w = np.arange(int(total.value), dtype=np.int64) - np.repeat(win_off[:-1], nw)
    n = np.repeat(rl, nw)
    start = w * W
    end = np.minimum(n, start + W) if W > 0 else n
    return win_off, start, end, int(total.value)


def autocorr_text(text, read_off, read_lens, k, D=4096, window=0, device=None, threads=1):
    """autocorr on reads given as one buffer with offsets and lengths, as the C-ABI takes them (gaps, padding and any order
    of offsets are allowed) -> formats.Autocorr"""
    import numpy as np
    from . import formats
    k, D, W = _autocorr_args(k, D, window, "autocorr")
    L = load()
    tb, ro, rl = _text_reads("autocorr", text, read_off, read_lens)
    win_off, start, end, windows = autocorr_layout(rl, W)
    cells = windows * D if windows * D <= AUTOCORR_CELLS_MAX else 0   # (over the cap: the library refuses before it writes)
    counts = np.zeros(max(cells, 1), dtype=np.int64)
    err = _err()
    if device is None:
        rc = L.sd_autocorr_host(tb or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, D, W, int(threads), counts.ctypes.data, err, 1024)
    else:
        rc = L.sd_autocorr_dev(tb or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, D, W, int(device), int(threads),
                               counts.ctypes.data, err, 1024)
    _text_check(rc, err)
    return formats.Autocorr(counts[:cells].reshape(windows, D), win_off, start, end, k)


def autocorr(reads, k, D=4096, window=0, device=None, threads=1):
    """The k-mer autocorrelation of every read against itself (include/sd_hip.h: sd_autocorr_*): counts[w, d - 1] = the
    positions i of window w whose k-mer recurs at i + d, neither copy holding a byte outside ACGT, for d = 1 .. D.  reads: a
    list of bytes / str, or a DeviceReads (then the kernels read the device text where it lies, on the reads' device).
    window: bases per window, 0 = the whole read.  device=None: host threads (sd_autocorr_host); else the kernels of
    csrc/sd_autocorr.hip on that device.  Both give the same integers.  -> formats.Autocorr"""
    if isinstance(reads, DeviceReads):
        return autocorr_device(reads, k, D, window).to_host(k, reads.read_lens, window)
    text, ro, rl = _reads_text(reads)
    return autocorr_text(text, ro, rl, k, D, window, device, threads)


class DeviceAutocorr(namedtuple("DeviceAutocorr", "counts win_off")):
    """The autocorrelation counts of a DeviceReads in device memory (autocorr_device): counts = int64 [windows, D], win_off =
    int64 [n + 1], torch tensors on the reads' device; nothing has been copied to the host."""
    __slots__ = ()

    def to_host(self, k, read_lens, window=0):
        """-> formats.Autocorr (waits for the device); read_lens and window: those of the call, for the windows' bounds"""
        from . import formats
        _, start, end, _ = autocorr_layout(read_lens, window)
        return formats.Autocorr(self.counts.cpu().numpy(), self.win_off.cpu().numpy(), start, end, k)


def autocorr_device(reads, k, D=4096, window=0, stream=None, counts=None):
    """autocorr on a DeviceReads, everything on the reads' device (sd_autocorr_reads_dev) -> DeviceAutocorr.  torch allocates
    the counters on `stream` (None: the device's current stream) -- or counts = an int64 tensor of windows x D elements on
    that device is used, whatever it holds -- and the library zeroes and fills them there; the call returns with the kernels
    in flight and nothing is copied to the host."""
    k, D, W = _autocorr_args(k, D, window, "autocorr_device")
    import torch
    L = load()
    dev = torch.device("cuda", reads.device)
    st = _torch_stream(torch, dev, stream)
    win_off, _, _, windows = autocorr_layout(reads.read_lens, W)
    if windows * D > AUTOCORR_CELLS_MAX:
        raise SdError(SD_ERR_PARAM, "autocorr_device: %d windows x %d lags, the cap is %d cells (AUTOCORR_CELLS_MAX): use longer "
                                    "windows, fewer lags or fewer reads per call" % (windows, D, AUTOCORR_CELLS_MAX))
    if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
        ev = torch.cuda.Event()
        ev.record(_torch_stream(torch, dev, reads.stream))
        st.wait_event(ev)
    with torch.cuda.stream(st):
        if counts is None:
            counts = torch.empty((windows, D), dtype=torch.int64, device=dev)
        elif counts.dtype != torch.int64 or counts.numel() != windows * D or counts.device != dev or not counts.is_contiguous():
            raise SdError(SD_ERR_PARAM, "autocorr_device: counts must be a contiguous int64 tensor of %d x %d elements on %s" % (windows, D, dev))
        d_off = torch.from_numpy(win_off).to(dev, non_blocking=True)
    err = C.create_string_buffer(1024)
    _text_check(L.sd_autocorr_reads_dev(C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n, k, D, W, dev.index or 0,
                                        C.c_void_p(st.cuda_stream), C.c_void_p(counts.data_ptr() if counts.numel() else 0), err, 1024), err)
    return DeviceAutocorr(counts.view(windows, D), d_off)


def autocorr_positions(read_lens, k, D, window=0):
    """positions[w, d - 1] = the i of window w with i <= n - d - k: what counts[w, d - 1] is out of (sd_autocorr_positions)"""
    import numpy as np
    k, D, W = _autocorr_args(k, D, window, "autocorr_positions")
    rl = np.ascontiguousarray(read_lens, dtype=np.int64).reshape(-1)
    windows = autocorr_layout(rl, W)[3]
    if windows * D > AUTOCORR_CELLS_MAX:
        raise SdError(SD_ERR_PARAM, "autocorr_positions: %d windows x %d lags, the cap is %d cells" % (windows, D, AUTOCORR_CELLS_MAX))
    out = np.zeros((windows, D), dtype=np.int64)
    _check(load().sd_autocorr_positions(rl.ctypes.data, len(rl), k, D, W, out.ctypes.data), "sd_autocorr_positions")
    return out


def autocorr_peaks(counts, lo=1, radius=8, peaks=8):
    """The peaks of every spectrum (row) of counts [windows, D] by the integer rule of csrc/sd_autocorr.hpp
    (sd_autocorr_peaks): lag d >= lo is a peak when its count is positive, no count within `radius` lags (and >= lo) is
    larger, and none of those at a smaller lag is equal.  -> (lag, count) int64 [windows, peaks], by count descending then
    lag ascending, 0-filled; lag[:, 0] is the period, 0 where a spectrum has no peak."""
    import numpy as np
    c = np.ascontiguousarray(counts, dtype=np.int64)
    if c.ndim == 1:
        c = c.reshape(1, -1)
    for name, v, low in (("lo", lo, 1), ("radius", radius, 0), ("peaks", peaks, 0)):
        _int_arg("autocorr_peaks", name, v, low, (1 << 31) - 1, ", %d or more" % low)
    if c.ndim != 2 or not 1 <= c.shape[1] <= AUTOCORR_DMAX:
        raise SdError(SD_ERR_PARAM, "autocorr_peaks: counts must be [windows, D] with 1 <= D <= %d" % AUTOCORR_DMAX)
    lag = np.zeros((c.shape[0], peaks), dtype=np.int64)
    cnt = np.zeros((c.shape[0], peaks), dtype=np.int64)
    _check(load().sd_autocorr_peaks(c.ctypes.data, c.shape[0], c.shape[1], lo, radius, peaks, lag.ctypes.data, cnt.ctypes.data),
           "sd_autocorr_peaks")
    return lag, cnt


def autocorr_seed(seq, k, p):
    """(s, run): the longest run of consecutive hits at lag p in seq starts at s and has run positions, the first of equal
    runs; (-1, 0) when there is no hit (sd_autocorr_seed)"""
    k, _, _ = _autocorr_args(k, 1, 0, "autocorr_seed")
    p = _int_arg("autocorr_seed", "p", p, 1, None, ", 1 or more", bools=True)   # (True has always been lag 1 here)
    sb = _b(seq)
    s, run = C.c_int64(0), C.c_int64(0)
    _check(load().sd_autocorr_seed(sb or b"N", len(sb), k, p, C.byref(s), C.byref(run)), "sd_autocorr_seed")
    return int(s.value), int(run.value)


def autocorr_seeds(reads, names, ac, lo=1, min_count=1, radius=8):
    """Seed monomers from the whole-read spectra of a formats.Autocorr: for every read whose spectrum has a period p (the
    first peak at a lag >= lo) with at least min_count hits, the p bases from the start s of the longest run of consecutive
    hits at lag p; a seed with a byte outside ACGT is dropped.  -> [(name, sequence)] with name =
    "{read}/{s}_{s + p} period={p} count={hits}", ready for a FASTA file that `--profile` then polishes."""
    out = []
    for r, (seq, name) in enumerate(zip(reads, names)):
        spec = ac.spectrum(r)
        lag, cnt = autocorr_peaks(spec, lo, radius, 1)
        p, c = int(lag[0, 0]), int(cnt[0, 0])
        if p <= 0 or c < min_count:
            continue
        sb = _b(seq)
        s, run = autocorr_seed(sb, ac.k, p)
        seed = sb[s:s + p] if s >= 0 else b""
        if len(seed) != p or seed.strip(b"ACGT"):
            continue
        out.append(("%s/%d_%d period=%d count=%d" % (name, s, s + p, p, c), seed.decode()))
    return out


def autocorr_rows(ac, names, read_lens, lo=1, radius=8, peaks=8):
    """The lines of <out>_autocorr.tsv for a formats.Autocorr -> [formats.AutocorrRow], one per (read, window)"""
    from . import formats
    lag, cnt = autocorr_peaks(ac.counts, lo, radius, max(peaks, 1))
    out = []
    for r, name in enumerate(names):
        n = int(read_lens[r])
        for w in ac.windows(r):
            ws, we = int(ac.win_start[w]), int(ac.win_end[w])
            p, c = int(lag[w, 0]), int(cnt[w, 0])
            pos = max(0, min(we, n - p - ac.k + 1) - ws) if p > 0 else 0
            pk = tuple((int(a), int(b)) for a, b in zip(lag[w, :peaks], cnt[w, :peaks]) if a > 0)
            out.append(formats.AutocorrRow(name, ws, we, ac.k, p, c, pos, pk))
    return out


def autocorr_spectrum_rows(ac, names, read_lens):
    """The lines of <out>_autocorr_spectrum.tsv -> [formats.AutocorrSpectrumRow]: every lag of every window with a count"""
    import numpy as np
    from . import formats
    out = []
    for r, name in enumerate(names):
        n = int(read_lens[r])
        for w in ac.windows(r):
            ws, we = int(ac.win_start[w]), int(ac.win_end[w])
            row = ac.counts[w]
            for d0 in np.nonzero(row)[0].tolist():
                d = d0 + 1
                out.append(formats.AutocorrSpectrumRow(name, ws, we, d, int(row[d0]), max(0, min(we, n - d - ac.k + 1) - ws)))
    return out


def autocorr_kernel_bench(reads, k, D=4096, window=0, device=0, warmup=2, reps=5):
    """sd_autocorr_kernel_bench -> {"prep_ms", "pairs_ms": [...], "launches", "workgroups", "cells", "words"}."""
    k, D, W = _autocorr_args(k, D, window, "autocorr_kernel_bench")
    text, ro, rl = _reads_text(reads)
    return _bench(load().sd_autocorr_kernel_bench, (text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, D, W, int(device), int(warmup),
                                                    int(reps)), ("prep_ms", "pairs_ms"), ("launches", "workgroups", "cells", "words"), reps)


MOTIF_BUILTIN = {"cenpb": "NTTCGNNNNANNCGGGN"}   # the CENP-B box of alpha-satellite monomers
MOTIF_LMAX = 64
MOTIF_EMAX = 7
MOTIF_MAX = 1024
MOTIF_ITEMS_MAX = 1 << 24
MOTIF_HITS_MAX = 1 << 28
MOTIF_TILE_WORDS = 256


def motif_hit_dtype():
    """sd_motif_hit (include/sd_hip.h) as a numpy dtype: 16 bytes"""
    import numpy as np
    return np.dtype([("start", "<i8"), ("read", "<i4"), ("motif", "<u2"), ("strand", "u1"), ("mismatches", "u1")])


def motif_request(motifs):
    """The motifs of a request -> (names, patterns).  motifs: a dict name -> pattern, or a list whose items are (name,
    pattern) pairs, built-in names (MOTIF_BUILTIN) or "NAME=PATTERN" strings, in request order."""
    if isinstance(motifs, dict):
        motifs = list(motifs.items())
    elif isinstance(motifs, (str, bytes)):
        motifs = [motifs]
    names, patterns = [], []
    for m in motifs:
        if isinstance(m, (tuple, list)) and len(m) == 2:
            name, pat = m
        else:
            spec = m.decode() if isinstance(m, bytes) else str(m)
            if "=" in spec:
                name, pat = spec.split("=", 1)
            elif spec in MOTIF_BUILTIN:
                name, pat = spec, MOTIF_BUILTIN[spec]
            else:
                raise SdError(SD_ERR_PARAM, "motif '%s' is neither NAME=PATTERN nor one of the built-in motifs (%s)"
                              % (spec, ", ".join(sorted(MOTIF_BUILTIN))))
        names.append(name.decode() if isinstance(name, bytes) else str(name))
        patterns.append(pat.decode() if isinstance(pat, bytes) else str(pat))
    return names, patterns


def _motif_mismatches(E, who):
    """an integer that fits the C type; the range 0 .. 7 is the library's to refuse, with its text"""
    return _int_arg(who, "mismatches", E, -(1 << 31), (1 << 31) - 1, " 0 .. %d" % MOTIF_EMAX)


MotifStrand = namedtuple("MotifStrand", "motif strand length constrained palindrome")


def motif_compile(motifs, E=0):
    """sd_motif_compile: the request checked -- names, patterns, E, the library's refusal as SdError -- and its
    pattern-strands -> (names, patterns, [MotifStrand]): two per motif (+ then -), one for a palindrome."""
    import numpy as np
    names, patterns = motif_request(motifs)
    E = _motif_mismatches(E, "motif_compile")
    n = len(names)
    table = np.zeros((2 * max(n, 1), 5), dtype=np.int32)
    ns = C.c_int32(0)
    err = _err()
    _text_check(load().sd_motif_compile(_strs(names), _strs(patterns), n, E, C.byref(ns), table.ctypes.data, err, 1024), err)
    return names, patterns, [MotifStrand(*(int(x) for x in row)) for row in table[:ns.value]]


def motif_info():
    """sd_motif_info -> {"tile": words of a workgroup's tile (64 starts each), "pattern_block": pattern-strands a workgroup
    takes, "launch_work": the most start x pattern-strand products of one launch, "launches": launches of the size and
    write kernels in this process so far}"""
    return _info(load().sd_motif_info, ("tile", "pattern_block", "launch_work", "launches"))


# ---- the two hit searches, motif and motif_edits: one implementation of each call, parameterised by a _HitSearch
# (csrc/sd_hits_job.hpp is the same frame on the other side of the C-ABI).  c: the prefix of the C functions; dtype: the hit
# record; result / device_result: the classes of formats and of this module the calls return; request(who, motifs, budget)
# -> (names, patterns), the request checked as the search checks it
_HitSearch = namedtuple("_HitSearch", "c dtype result device_result request")


def _hits_array(s, buf, n):
    import numpy as np
    return np.frombuffer(buf, dtype=s.dtype()).copy() if n else np.zeros(0, dtype=s.dtype())


def _hits_text(s, who, text, read_off, read_lens, motifs, budget, device, threads):
    import numpy as np
    from . import formats
    names, patterns = s.request(who, motifs, budget)
    L = load()
    tb, ro, rl = _text_reads(who, text, read_off, read_lens)
    per = np.zeros((len(rl), len(names), 2), dtype=np.int64)
    out, n = C.c_void_p(0), C.c_int64(0)
    err = _err()
    fn, where = (getattr(L, s.c + "_host"), int(threads)) if device is None else (getattr(L, s.c + "_dev"), int(device))
    _text_check(fn(tb or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), _strs(patterns), len(names), budget, where,
                   C.byref(out), C.byref(n), per.ctypes.data, err, 1024), err)
    try:
        hits = _hits_array(s, C.string_at(out.value, 16 * n.value), n.value)
    finally:
        L.sd_free(out)
    return getattr(formats, s.result)(hits, per, names, patterns, budget)


class _DeviceHits:
    """what DeviceMotifs and DeviceMotifEdits share: (hits, per, n_hits, names, patterns, budget) and the way to the host"""
    __slots__ = ()

    def to_host(self):
        """-> formats.Motifs / formats.MotifEdits (waits for the device)"""
        from . import formats
        s = _HIT_SEARCH[self._search]
        return getattr(formats, s.result)(_hits_array(s, self.hits.cpu().numpy().tobytes(), self.n_hits), self.per.cpu().numpy(),
                                          self.names, self.patterns, self[5])


def _hits_device(s, who, reads, motifs, budget, stream, hits, per):
    names, patterns = s.request(who, motifs, budget)
    L = load()
    torch, dev, st = _device_frame(reads.device, stream)
    if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
        ev = torch.cuda.Event()
        ev.record(_torch_stream(torch, dev, reads.stream))
        st.wait_event(ev)
    nm = len(names)
    if per is None:
        with torch.cuda.stream(st):
            per = torch.empty((reads.n, nm, 2), dtype=torch.int64, device=dev)
    elif per.dtype != torch.int64 or per.numel() != reads.n * nm * 2 or per.device != dev or not per.is_contiguous():
        raise SdError(SD_ERR_PARAM, "%s: per must be a contiguous int64 tensor of %d x %d x 2 elements on %s" % (who, reads.n, nm, dev))
    lead = (C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n, _strs(patterns), nm, budget, dev.index or 0, C.c_void_p(st.cuda_stream))
    n = C.c_int64(0)
    err = _err()
    _text_check(getattr(L, s.c + "_reads_size_dev")(*lead, _dptr(per), C.byref(n), err, 1024), err)
    if hits is None:
        with torch.cuda.stream(st):
            hits = torch.empty((n.value, 16), dtype=torch.uint8, device=dev)
    elif hits.dtype != torch.uint8 or hits.device != dev or not hits.is_contiguous():
        raise SdError(SD_ERR_PARAM, "%s: hits must be a contiguous uint8 tensor on %s" % (who, dev))
    _text_check(getattr(L, s.c + "_reads_write_dev")(*lead, _dptr(hits), hits.numel() // 16, err, 1024), err)
    return s.device_result(hits.view(-1)[:16 * n.value].view(n.value, 16), per.view(reads.n, nm, 2), int(n.value), names, patterns, budget)


def _hits_kernel_bench(s, who, reads, motifs, budget, device, warmup, reps):
    names, patterns = s.request(who, motifs, budget)
    text, ro, rl = _reads_text(reads)
    return _bench(getattr(load(), s.c + "_kernel_bench"), (text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), _strs(patterns), len(names), budget,
                                                           int(device), int(warmup), int(reps)), ("prep_ms", "size_ms", "write_ms"),
                  ("launches", "items", "hits", "words"), reps)


def motif_text(text, read_off, read_lens, motifs, E=0, device=None, threads=1):
    """motif on reads given as one buffer with offsets and lengths, as the C-ABI takes them (gaps, padding and any order
    of offsets are allowed) -> formats.Motifs"""
    return _hits_text(_HIT_SEARCH["motif"], "motif", text, read_off, read_lens, motifs, E, device, threads)


def motif(reads, motifs, E=0, device=None, threads=1):
    """The hits of IUPAC motifs on both strands of every read (include/sd_hip.h: sd_motif_*): Hamming matches with at most E
    mismatches at the constrained positions, every hit reported.  reads: a list of bytes / str, or a DeviceReads (then the
    kernels read the device text where it lies).  motifs: see motif_request.  device=None: host threads (sd_motif_host);
    else the kernels of csrc/sd_motif.hip on that device.  Both give the same arrays.  -> formats.Motifs"""
    if isinstance(reads, DeviceReads):
        return motif_device(reads, motifs, E).to_host()
    text, ro, rl = _reads_text(reads)
    return motif_text(text, ro, rl, motifs, E, device, threads)


class DeviceMotifs(_DeviceHits, namedtuple("DeviceMotifs", "hits per n_hits names patterns E")):
    """The motif hits of a DeviceReads in device memory (motif_device): hits = uint8 [n_hits, 16], the sd_motif_hit records
    in canonical order; per = int64 [reads, motifs, 2]; torch tensors on the reads' device.  names, patterns, E: the request
    they answer."""
    __slots__ = ()
    _search = "motif"


def motif_device(reads, motifs, E=0, stream=None, hits=None, per=None):
    """motif on a DeviceReads, everything on the reads' device (sd_motif_reads_size_dev / sd_motif_reads_write_dev) ->
    DeviceMotifs(hits, per, n_hits, ...).  torch allocates the results on `stream` (None: the device's current stream) -- or hits (uint8, at least
    16 bytes per hit) and per (int64, reads x motifs x 2) are used, whatever they hold -- and the library fills them there.
    The host waits once, for the number of hits; the call returns with the write kernels in flight."""
    return _hits_device(_HIT_SEARCH["motif"], "motif_device", reads, motifs, E, stream, hits, per)


def motif_kernel_bench(reads, motifs, E=0, device=0, warmup=2, reps=5):
    """sd_motif_kernel_bench -> {"prep_ms", "size_ms", "write_ms": [...], "launches", "items", "hits", "words"}."""
    return _hits_kernel_bench(_HIT_SEARCH["motif"], "motif_kernel_bench", reads, motifs, E, device, warmup, reps)


MOTIF_KMAX = 7
MOTIF_EDIT_TILE_WORDS = 256


def motif_edit_hit_dtype():
    """sd_motif_edit_hit (include/sd_hip.h) as a numpy dtype: 16 bytes; strand_edits = strand << 7 | edits"""
    import numpy as np
    return np.dtype([("start", "<i8"), ("read", "<i4"), ("motif", "<u2"), ("length", "u1"), ("strand_edits", "u1")])


def motif_edits_request(motifs, K, who):
    """The request of an edit call checked on the host -- names and patterns as motif_compile checks them, K an integer
    0 .. MOTIF_KMAX, every motif with more than K constrained positions -> (names, patterns)"""
    names, patterns, strands = motif_compile(motifs, 0)
    _int_arg(who, "edits", K, 0, MOTIF_KMAX)
    for s in strands:
        if s.constrained <= K:
            raise SdError(SD_ERR_PARAM, "%s: motif '%s': %d constrained positions with %d edits allowed: it would hit everywhere"
                          % (who, names[s.motif], s.constrained, K))
    return names, patterns


def motif_edits_info():
    """sd_motif_edit_info -> {"stretch": consecutive ends a lane owns, "tile": words of a workgroup's tile (256 stretches),
    "pattern_block": pattern-strands a workgroup takes, "launch_work": the most end x pattern-strand products of one launch,
    "launches": launches of the size and write kernels in this process so far, "launch_wg": work items of one launch}"""
    return _info(load().sd_motif_edit_info, ("stretch", "tile", "pattern_block", "launch_work", "launches", "launch_wg"))


def motif_edits_text(text, read_off, read_lens, motifs, K, device=None, threads=1):
    """motif_edits on reads given as one buffer with offsets and lengths, as the C-ABI takes them (gaps, padding and any
    order of offsets are allowed) -> formats.MotifEdits"""
    return _hits_text(_HIT_SEARCH["motif_edits"], "motif_edits", text, read_off, read_lens, motifs, K, device, threads)


def motif_edits(reads, motifs, K, device=None, threads=1):
    """The hits of IUPAC motifs on both strands of every read with up to K edits -- substitutions at the constrained
    positions, inserted text bytes, deleted pattern codes (include/sd_hip.h: sd_motif_edit_*; csrc/sd_motif_edit.hpp holds
    the rule).  reads: a list of bytes / str, or a DeviceReads (then the kernels read the device text where it lies).
    motifs: see motif_request.  device=None: host threads (sd_motif_edit_host); else the kernels of csrc/sd_motif_edit.hip on
    that device.  Both give the same arrays.  -> formats.MotifEdits"""
    if isinstance(reads, DeviceReads):
        return motif_edits_device(reads, motifs, K).to_host()
    text, ro, rl = _reads_text(reads)
    return motif_edits_text(text, ro, rl, motifs, K, device, threads)


class DeviceMotifEdits(_DeviceHits, namedtuple("DeviceMotifEdits", "hits per n_hits names patterns K")):
    """The edit hits of a DeviceReads in device memory (motif_edits_device): hits = uint8 [n_hits, 16], the
    sd_motif_edit_hit records in canonical order; per = int64 [reads, motifs, 2]; torch tensors on the reads' device."""
    __slots__ = ()
    _search = "motif_edits"


def motif_edits_device(reads, motifs, K, stream=None, hits=None, per=None):
    """motif_edits on a DeviceReads, everything on the reads' device (sd_motif_edit_reads_size_dev / _write_dev) ->
    DeviceMotifEdits(hits, per, n_hits, ...).  torch allocates the results on `stream` (None: the device's current stream)
    -- or hits (uint8, at least 16 bytes per hit) and per (int64, reads x motifs x 2) are used, whatever they hold -- and
    the library fills them there.  The host waits once, for the number of hits; the call returns with the write kernels in
    flight."""
    return _hits_device(_HIT_SEARCH["motif_edits"], "motif_edits_device", reads, motifs, K, stream, hits, per)


def motif_edits_kernel_bench(reads, motifs, K, device=0, warmup=2, reps=5):
    """sd_motif_edit_kernel_bench -> {"prep_ms", "size_ms", "write_ms": [...], "launches", "items", "hits", "words"}."""
    return _hits_kernel_bench(_HIT_SEARCH["motif_edits"], "motif_edits_kernel_bench", reads, motifs, K, device, warmup, reps)


_HIT_SEARCH = {
    "motif": _HitSearch("sd_motif", motif_hit_dtype, "Motifs", DeviceMotifs, lambda who, motifs, E: motif_compile(motifs, E)[:2]),
    "motif_edits": _HitSearch("sd_motif_edit", motif_edit_hit_dtype, "MotifEdits", DeviceMotifEdits, lambda who, motifs, K: motif_edits_request(motifs, K, who)),
}


# ---- cyclic pairs and the merge of seed monomers (csrc/sd_cyclic.hpp holds the rule) ---------------------------------------
CYCLIC_QMAX = 2048        # SD_CYCLIC_QMAX: the longest query of the lane kernel (one pair to a lane)
CYCLIC_QMAX_LONG = 16384  # SD_CYCLIC_QMAX_LONG: the longest query the device takes (the team kernel: a query across 16 .. 64 lanes)
CYCLIC_TEAM_CLASSES = tuple((K, L) for L in (16, 32, 64) for K in (1, 2, 3, 4))   # words per lane x lanes: 64 K L rows
CYCLIC_TMAX = 65535       # SD_CYCLIC_TMAX: the longest target the device takes
CYCLIC_PAIRS_MAX = 1 << 24
CYCLIC_N_MAX = 1 << 20
CYCLIC_LAUNCH_WG_MIN = 1024   # SD_CYCLIC_LAUNCH_WG_MIN: a launch is not closed by its step bound below this many workgroups


def cyclic_info():
    """sd_cyclic_info -> {"lmax_query": the lane kernel's limit in bases (cyclic_long_info has the team kernel's),
    "lmax_target": the device's limit, "launch_work": the step bound of a launch of either pair kernel, "launches": of the
    lane kernel in this process so far, "pairs_max": pairs of a cyclic_pairs
    call, "block": the default block of cyclic_merge}.  The bound of a launch is compound: at most launch_work word steps
    (columns x words x pairs) or CYCLIC_LAUNCH_WG_MIN workgroups, whichever is more, so launch_work is the most only while
    workgroups are small (include/sd_hip.h has the largest launch there can be)."""
    return _info(load().sd_cyclic_info, ("lmax_query", "lmax_target", "launch_work", "launches", "pairs_max", "block"))


def _cyclic_seqs(who, seqs, names=None):
    """the sequences of a cyclic call as (text, offsets, lengths), each upper-case ACGT of length >= 1 -- refused here by
    index, and by name where there is one, before the library is called"""
    sb = [_b(s) for s in seqs]
    for i, s in enumerate(sb):
        tag = "sequence %d" % i + (" (%s)" % names[i] if names is not None else "")
        if not s:
            raise SdError(SD_ERR_PARAM, "%s: %s is empty" % (who, tag))
        if s.strip(b"ACGT"):
            raise SdError(SD_ERR_PARAM, "%s: %s holds a byte outside ACGT" % (who, tag))
    return _reads_text(sb)


def _cyclic_index(who, name, idx, n):
    import numpy as np
    a = np.arange(n, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    if len(a) and (int(a.min()) < 0 or int(a.max()) >= n):
        raise SdError(SD_ERR_PARAM, "%s: %s holds an index outside the %d sequences" % (who, name, n))
    return a


def _cyclic_call(who, seqs, queries, targets):
    text, ro, rl = _cyclic_seqs(who, seqs)
    qi, ti = _cyclic_index(who, "queries", queries, len(rl)), _cyclic_index(who, "targets", targets, len(rl))
    if len(qi) * len(ti) > CYCLIC_PAIRS_MAX:
        raise SdError(SD_ERR_PARAM, "%s: %d x %d pairs, the cap is %d per call" % (who, len(qi), len(ti), CYCLIC_PAIRS_MAX))
    return text, ro, rl, qi, ti


def cyclic_pairs(seqs, queries=None, targets=None, device=None, threads=1):
    """Cyclic pairs: for every query q and target t of `seqs` (indices; None = all), the smallest edit distance of q to a
    substring of t written twice, on either strand, and where that fit ends (include/sd_hip.h: sd_cyclic_pairs_*) ->
    formats.CyclicPairs(dist, end, strand, phase), int32 / int32 / uint8 / int32 arrays [queries, targets]; phase =
    (end + 1) mod |t|, where in t (on that strand) a query that is a whole period begins.
    device=None: host threads (sd_cyclic_pairs_host); else the kernels of csrc/sd_cyclic.hip on that device -- queries of up
    to 2 048 bp one pair to a lane, of up to 16 384 bp one query across a team of lanes -- with the pairs beyond its limits
    (query > 16 384 bp, target > 65 535 bp) on `threads` host threads.  Both give the same arrays."""
    import numpy as np
    from . import formats
    text, ro, rl, qi, ti = _cyclic_call("cyclic_pairs", seqs, queries, targets)
    m, k = len(qi), len(ti)
    dist, end, strand = np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.uint8)
    L, err = load(), _err()
    lead = (text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k)
    out = (dist.ctypes.data, end.ctypes.data, strand.ctypes.data, err, len(err))
    if device is None:
        rc = L.sd_cyclic_pairs_host(*lead, int(threads), *out)
    else:
        rc = L.sd_cyclic_pairs_dev(*lead, int(device), int(threads), *out)
    _text_check(rc, err, "cyclic_pairs")
    tl = rl[ti].astype(np.int32) if k else np.zeros(0, dtype=np.int32)
    phase = (end + 1) % tl[None, :] if m and k else np.zeros((m, k), dtype=np.int32)
    return formats.CyclicPairs(dist, end, strand, phase.astype(np.int32))


def cyclic_merge(seqs, weights=None, P=85, block=None, device=None, threads=1, names=None):
    """The merge of sequences that are the same monomer up to rotation, strand and (100 - P) percent of edits
    (csrc/sd_cyclic.hpp has the rule; sd_cyclic_merge_*): visited by weight descending (None: all 0), then index ascending,
    a sequence joins the closest centre it is close to, or becomes the next centre -> formats.CyclicMerge(cluster, centre,
    dist, end, strand, phase, n_clusters), arrays per sequence: cluster 0-based in order of creation, centre the index of
    the cluster's centre, the rest the sequence's pair in its centre.  block: sequences per step (None: the default); the
    result does not depend on it.  device as in cyclic_pairs.  names: used in refusals only."""
    import numpy as np
    from . import formats
    who = "cyclic_merge"
    P = _int_arg(who, "P", P, 1, 100)
    block = 0 if block is None else _int_arg(who, "block", block, 1, None, ", 1 or more")
    text, ro, rl = _cyclic_seqs(who, seqs, names)
    n = len(rl)
    if n > CYCLIC_N_MAX:
        raise SdError(SD_ERR_PARAM, "%s: %d sequences, the cap is %d" % (who, n, CYCLIC_N_MAX))
    w = np.zeros(n, dtype=np.int64) if weights is None else np.ascontiguousarray(weights, dtype=np.int64).reshape(-1)
    if len(w) != n:
        raise SdError(SD_ERR_PARAM, "%s: %d weights for %d sequences" % (who, len(w), n))
    cluster, centre, dist, end = (np.zeros(n, dtype=np.int32) for _ in range(4))
    strand = np.zeros(n, dtype=np.uint8)
    nc = C.c_int32(0)
    L, err = load(), _err()
    lead = (text or b"N", ro.ctypes.data, rl.ctypes.data, n, w.ctypes.data, P, min(block, 1 << 30))
    out = (cluster.ctypes.data, centre.ctypes.data, dist.ctypes.data, end.ctypes.data, strand.ctypes.data, C.byref(nc), err, len(err))
    if device is None:
        rc = L.sd_cyclic_merge_host(*lead, int(threads), *out)
    else:
        rc = L.sd_cyclic_merge_dev(*lead, int(device), int(threads), *out)
    _text_check(rc, err, who)
    phase = ((end + 1) % rl[centre].astype(np.int32)).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    return formats.CyclicMerge(cluster, centre, dist, end, strand, phase, int(nc.value))


def cyclic_canon(seq):
    """(record, rotation, strand): the lexicographically smallest among all rotations of seq and of its reverse complement
    = s[rotation:] + s[:rotation] with s = seq (strand 0) or its reverse complement (strand 1) (sd_cyclic_canon)"""
    sb = _b(seq)
    if not sb or sb.strip(b"ACGT"):
        raise SdError(SD_ERR_PARAM, "cyclic_canon: the sequence is empty or holds a byte outside ACGT")
    out = C.create_string_buffer(len(sb))
    rot, strand = C.c_int64(0), C.c_int32(0)
    _check(load().sd_cyclic_canon(sb, len(sb), out, C.byref(rot), C.byref(strand)), "sd_cyclic_canon")
    return out.raw.decode(), int(rot.value), int(strand.value)


def cyclic_kernel_bench(seqs, queries=None, targets=None, device=0, warmup=2, reps=5, variant=0, arrays=False):
    """sd_cyclic_kernel_bench -> {"pairs_ms": [...], "launches", "pairs", "steps", "workgroups"}: the lane kernel's launches
    of cyclic_pairs(seqs, queries, targets, device) between two events; pairs and steps (columns x words x pairs) on the
    device.  Queries of more than CYCLIC_QMAX bp are not computed here: cyclic_long_kernel_bench times the team kernel.  variant: 0 = the kernels the library chooses, 1 = 64-bit words throughout, 2 = 32-bit halves up to four words.
    arrays=True: also "dist", "end", "strand" of the timed variant, as cyclic_pairs gives them."""
    import numpy as np
    text, ro, rl, qi, ti = _cyclic_call("cyclic_kernel_bench", seqs, queries, targets)
    variant = _int_arg("cyclic_kernel_bench", "variant", variant, 0, 2)
    m, k = len(qi), len(ti)
    ms, info = (C.c_float * reps)(), (C.c_int64 * 4)()
    dist, end, strand = np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.uint8)
    _check(load().sd_cyclic_kernel_bench(text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k, int(device),
                                         variant, int(warmup), int(reps), ms, info, dist.ctypes.data, end.ctypes.data, strand.ctypes.data),
           "sd_cyclic_kernel_bench")
    out = {"pairs_ms": [float(x) for x in ms]}
    out.update(zip(("launches", "pairs", "steps", "workgroups"), (int(x) for x in info)))
    if arrays:
        out.update(dist=dist, end=end, strand=strand)
    return out


def cyclic_long_info():
    """sd_cyclic_long_info -> {"lmax_query": the team kernel's limit in bases (CYCLIC_QMAX_LONG), "launches": of the team
    kernel in this process so far, "classes": the instantiated (K, L), "teams_per_wave": queries of a wave at L = 16}"""
    return _info(load().sd_cyclic_long_info, ("lmax_query", "launches", "classes", "teams_per_wave"))


def cyclic_team_class(length):
    """(K, L) of the team kernel for a query of `length` bases: the class of smallest K * L that holds it, the larger K of
    equal ones (csrc/sd_cyclic.hpp: cyclic_team_class); None beyond CYCLIC_QMAX_LONG"""
    words = (int(length) + 63) // 64
    fit = [(K * L, -K, K, L) for K, L in CYCLIC_TEAM_CLASSES if K * L >= words]
    return min(fit)[2:] if fit else None


def _cyclic_team_args(who, K, L, rl, qi):
    """a forced class, refused as the library refuses it"""
    if (K, L) not in CYCLIC_TEAM_CLASSES:
        raise SdError(SD_ERR_PARAM, "%s: K = %r, L = %r is no class of the team kernel (K 1 .. 4 words, L 16, 32 or 64 lanes)" % (who, K, L))
    for a, q in enumerate(qi):
        if rl[q] > 64 * K * L:
            raise SdError(SD_ERR_PARAM, "%s: query %d has %d bases, the class of %d words x %d lanes holds %d" % (who, a, rl[q], K, L, 64 * K * L))


def cyclic_pairs_team_host(seqs, queries=None, targets=None, K=4, L=64, threads=1):
    """sd_cyclic_pairs_team_host: cyclic_pairs by the team kernel's schedule of class (K, L) run on the host -- L lanes in
    lock step, K words each, the carry and the column's symbol handed down one lane per step -> formats.CyclicPairs, the
    arrays of cyclic_pairs.  Needs no device.  Refuses a (K, L) outside CYCLIC_TEAM_CLASSES and a query of more than
    64 * K * L bases (the library's line, SD_ERR_PARAM)."""
    import numpy as np
    from . import formats
    who = "cyclic_pairs_team_host"
    text, ro, rl, qi, ti = _cyclic_call(who, seqs, queries, targets)
    m, k = len(qi), len(ti)
    dist, end, strand = np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.uint8)
    err = _err()
    rc = load().sd_cyclic_pairs_team_host(text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k,
                                          _int_arg(who, "K", K, 0, 1 << 30), _int_arg(who, "L", L, 0, 1 << 30), int(threads),
                                          dist.ctypes.data, end.ctypes.data, strand.ctypes.data, err, len(err))
    _text_check(rc, err, who)
    tl = rl[ti].astype(np.int32) if k else np.zeros(0, dtype=np.int32)
    phase = (end + 1) % tl[None, :] if m and k else np.zeros((m, k), dtype=np.int32)
    return formats.CyclicPairs(dist, end, strand, phase.astype(np.int32))


def cyclic_long_kernel_bench(seqs, queries=None, targets=None, device=0, K=0, L=0, warmup=2, reps=5, arrays=False):
    """sd_cyclic_long_kernel_bench -> {"pairs_ms": [...], "launches", "pairs", "steps", "workgroups"}: the team kernel's
    launches between two events; steps = columns x words x pairs with pad words and ramp steps counted.  K = L = 0: the
    queries of CYCLIC_QMAX + 1 .. CYCLIC_QMAX_LONG bp in the library's classes; else every query of the call in class
    (K, L), short ones included -- a (K, L) outside CYCLIC_TEAM_CLASSES or a query of more than 64 * K * L bases is refused
    before the device is touched.  arrays=True: also "dist", "end", "strand" (pairs of other queries are not computed)."""
    import numpy as np
    who = "cyclic_long_kernel_bench"
    text, ro, rl, qi, ti = _cyclic_call(who, seqs, queries, targets)
    K, L = _int_arg(who, "K", K, 0, 1 << 30), _int_arg(who, "L", L, 0, 1 << 30)
    if (K, L) != (0, 0):
        _cyclic_team_args(who, K, L, rl, qi)
    m, k = len(qi), len(ti)
    ms, info = (C.c_float * reps)(), (C.c_int64 * 4)()
    dist, end, strand = np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.uint8)
    _check(load().sd_cyclic_long_kernel_bench(text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), qi.ctypes.data, ti.ctypes.data, m, k, int(device),
                                              K, L, int(warmup), int(reps), ms, info, dist.ctypes.data, end.ctypes.data, strand.ctypes.data),
           "sd_cyclic_long_kernel_bench")
    out = {"pairs_ms": [float(x) for x in ms]}
    out.update(zip(("launches", "pairs", "steps", "workgroups"), (int(x) for x in info)))
    if arrays:
        out.update(dist=dist, end=end, strand=strand)
    return out


DOTPLOT_KMAX = 32
DOTPLOT_WMAX = 1 << 30
DOTPLOT_MMAX = 1 << 20
DOTPLOT_BMAX = 1 << 30
DOTPLOT_CELLS_MAX = 1 << 27
DOTPLOT_SET_MAX = 4096


def _dotplot_args(k, W, B, M, who):
    """1 <= k <= 32, 1 <= W <= 2^30, 0 <= B <= 2^30, 1 <= M <= 2^20, refused here before any array is made or any device
    is touched"""
    return (_int_arg(who, "k", k, 1, DOTPLOT_KMAX), _int_arg(who, "W", W, 1, DOTPLOT_WMAX), _int_arg(who, "B", B, 0, DOTPLOT_BMAX),
            _int_arg(who, "M", M, 1, DOTPLOT_MMAX))


def dotplot_info():
    """sd_dotplot_info -> {"tile": positions of a tile of the counting pass, "jseg": cells of a row a workgroup of the pair
    kernel takes, "set_max", "launch_work": the most pair-elements of one launch of the pair kernel, "cells_max",
    "launches": its launches in this process so far}"""
    return _info(load().sd_dotplot_info, ("tile", "jseg", "set_max", "launch_work", "cells_max", "launches"))


def dotplot_hash(x):
    """h(x) of the selection rule, the splitmix64 finaliser (sd_dotplot_hash)"""
    return int(load().sd_dotplot_hash(C.c_uint64(x & ((1 << 64) - 1))))


def dotplot_layout(read_lens, W, B=0):
    """The windows and cells of reads of the given lengths (sd_dotplot_layout) -> (win_off, cell_off int64 [n + 1], windows,
    cells): read r owns the windows win_off[r] .. win_off[r + 1] and the cells cell_off[r] .. cell_off[r + 1]."""
    import numpy as np
    _, W, B, _ = _dotplot_args(1, W, B, 1, "dotplot_layout")
    rl = np.ascontiguousarray(read_lens, dtype=np.int64).reshape(-1)
    win_off = np.zeros(len(rl) + 1, dtype=np.int64)
    cell_off = np.zeros(len(rl) + 1, dtype=np.int64)
    nw, nc = C.c_int64(0), C.c_int64(0)
    _check(load().sd_dotplot_layout(rl.ctypes.data, len(rl), W, B, win_off.ctypes.data, cell_off.ctypes.data, C.byref(nw), C.byref(nc)),
           "sd_dotplot_layout: a negative read length, or 2^62 windows or cells, or more")
    return win_off, cell_off, int(nw.value), int(nc.value)


def _dotplot_cells_check(who, windows, cells):
    if cells > DOTPLOT_CELLS_MAX:
        raise SdError(SD_ERR_PARAM, "%s: %d windows make %d cells, the cap is %d (SD_DOTPLOT_CELLS_MAX): use longer windows, a band "
                                    "or fewer reads per call" % (who, windows, cells, DOTPLOT_CELLS_MAX))


def dotplot_text(text, read_off, read_lens, k, W, B=0, M=1, rc=False, device=None, threads=1):
    """dotplot on reads given as one buffer with offsets and lengths, as the C-ABI takes them (gaps, padding and any order of
    offsets are allowed) -> formats.Dotplot"""
    import numpy as np
    from . import formats
    k, W, B, M = _dotplot_args(k, W, B, M, "dotplot")
    L = load()
    tb, ro, rl = _text_reads("dotplot", text, read_off, read_lens)
    win_off, cell_off, windows, cells = dotplot_layout(rl, W, B)
    _dotplot_cells_check("dotplot", windows, cells)
    kmers, shared = np.zeros(max(windows, 1), dtype=np.int32), np.zeros(max(cells, 1), dtype=np.int32)
    kmers_rc, shared_rc = (np.zeros_like(kmers), np.zeros_like(shared)) if rc else (None, None)
    ptr = lambda a: a.ctypes.data if a is not None else None
    err = _err()
    if device is None:
        e = L.sd_dotplot_host(tb or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, W, B, M, int(bool(rc)), int(threads), ptr(kmers),
                              ptr(kmers_rc), ptr(shared), ptr(shared_rc), err, 1024)
    else:
        e = L.sd_dotplot_dev(tb or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, W, B, M, int(bool(rc)), int(device), ptr(kmers),
                             ptr(kmers_rc), ptr(shared), ptr(shared_rc), err, 1024)
    _text_check(e, err)
    return formats.Dotplot(kmers[:windows], kmers_rc[:windows] if rc else None, shared[:cells], shared_rc[:cells] if rc else None,
                           win_off, cell_off, rl.copy(), k, W, B, M)


def dotplot(reads, k, W, B=0, M=1, rc=False, device=None, threads=1):
    """The windowed k-mer identity of every read against itself (include/sd_hip.h: sd_dotplot_*): the read cut into windows
    of W bases, the cell (i, j), j <= i (i - j <= B when B > 0), = the distinct selected k-mers windows i and j share, with
    rc also those of window i whose reverse complement lies in window j.  M: keep a code when h(code) % M == 0.  reads: a
    list of bytes / str, or a DeviceReads (then the kernels read the device text where it lies).  device=None: host threads
    (sd_dotplot_host); else the kernels of csrc/sd_dotplot.hip on that device.  Both give the same integers.
    -> formats.Dotplot"""
    if isinstance(reads, DeviceReads):
        return dotplot_device(reads, k, W, B, M, rc).to_host(reads.read_lens, k, W, B, M)
    text, ro, rl = _reads_text(reads)
    return dotplot_text(text, ro, rl, k, W, B, M, rc, device, threads)


class DeviceDotplot(namedtuple("DeviceDotplot", "kmers kmers_rc shared shared_rc win_off cell_off")):
    """The dotplot of a DeviceReads in device memory (dotplot_device): kmers, kmers_rc int32 [windows], shared, shared_rc
    int32 [cells] (the two reverse-strand tensors None without rc), win_off, cell_off int64 [n + 1], torch tensors on the
    reads' device."""
    __slots__ = ()

    def to_host(self, read_lens, k, W, B=0, M=1):
        """-> formats.Dotplot (waits for the device)"""
        import numpy as np
        from . import formats
        h = lambda t: t.cpu().numpy() if t is not None else None
        return formats.Dotplot(h(self.kmers), h(self.kmers_rc), h(self.shared), h(self.shared_rc), h(self.win_off), h(self.cell_off),
                               np.asarray(read_lens, dtype=np.int64), k, W, B, M)


def dotplot_device(reads, k, W, B=0, M=1, rc=False, stream=None):
    """dotplot on a DeviceReads (or a list of bytes / str, uploaded first), everything on the reads' device
    (sd_dotplot_reads_dev) -> DeviceDotplot.  torch allocates the results on `stream` (None: the device's current stream)
    and the library fills them there.  The host waits once, for the counting pass's summary; the call returns with the other
    kernels in flight and no result is copied to the host."""
    k, W, B, M = _dotplot_args(k, W, B, M, "dotplot_device")
    import torch
    L = load()
    if not isinstance(reads, DeviceReads):
        import numpy as np
        rs = [_b(s) for s in reads]
        flat = np.frombuffer(b"".join(rs) or b"N", dtype=np.uint8).copy()   # (back to back; one byte when there is no base)
        reads = DeviceReads(torch.from_numpy(flat).to("cuda"), [len(s) for s in rs])
    dev = torch.device("cuda", reads.device)
    st = _torch_stream(torch, dev, stream)
    win_off, cell_off, windows, cells = dotplot_layout(reads.read_lens, W, B)
    _dotplot_cells_check("dotplot_device", windows, cells)
    if reads.stream != st.cuda_stream:   # the reads' bytes were produced on another stream: st waits for it
        ev = torch.cuda.Event()
        ev.record(_torch_stream(torch, dev, reads.stream))
        st.wait_event(ev)
    with torch.cuda.stream(st):
        kmers = torch.empty(windows, dtype=torch.int32, device=dev)
        shared = torch.empty(cells, dtype=torch.int32, device=dev)
        kmers_rc, shared_rc = (torch.empty_like(kmers), torch.empty_like(shared)) if rc else (None, None)
        d_win = torch.from_numpy(win_off).to(dev, non_blocking=True)
        d_cell = torch.from_numpy(cell_off).to(dev, non_blocking=True)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)
    err = C.create_string_buffer(1024)
    _text_check(L.sd_dotplot_reads_dev(C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n, k, W, B, M, int(bool(rc)), dev.index or 0,
                                       C.c_void_p(st.cuda_stream), ptr(kmers), ptr(kmers_rc), ptr(shared), ptr(shared_rc), err, 1024), err)
    return DeviceDotplot(kmers, kmers_rc, shared, shared_rc, d_win, d_cell)


def dotplot_kernel_bench(reads, k, W, B=0, M=1, rc=False, device=0, warmup=2, reps=5):
    """sd_dotplot_kernel_bench -> {"count_ms", "sets_ms", "pairs_ms": [...], "launches", "workgroups", "cells", "windows",
    "selected", "largest"}."""
    k, W, B, M = _dotplot_args(k, W, B, M, "dotplot_kernel_bench")
    text, ro, rl = _reads_text(reads)
    return _bench(load().sd_dotplot_kernel_bench, (text or b"N", ro.ctypes.data, rl.ctypes.data, len(rl), k, W, B, M, int(bool(rc)),
                                                   int(device), int(warmup), int(reps)), ("count_ms", "sets_ms", "pairs_ms"),
                  ("launches", "workgroups", "cells", "windows", "selected", "largest"), reps)


SPLIT_KMAX = 64
SPLIT_LMAX = 512
SPLIT_NMAX = 1 << 26


def _split_args(R, K, min_size, max_iter, who):
    """R, min_size, max_iter >= 1 and 1 <= K <= 64, refused here before any array is made or any device is touched"""
    for name, v in (("R", R), ("min_size", min_size), ("max_iter", max_iter)):
        _int_arg(who, name, v, 1, (1 << 31) - 1, ", 1 or more")
    return R, _int_arg(who, "K", K, 1, SPLIT_KMAX), min_size, max_iter


def _split_percent(P, who):
    return _int_arg(who, "P", P, 1, 100, " 1 .. 100 (a percentage of the monomer's length)")


def split_radius(P, L):
    """--split P: the radius of a monomer of L bases, max(1, ceil(P L / 100)) (csrc/sd_split.hpp: split_radius)"""
    return max(1, (int(P) * int(L) + 99) // 100)


def split_info():
    """sd_split_info -> {"kmax", "lmax": the longest monomer of the kernels, "nmax": the most member rows of a monomer,
    "launches": launches of the assign kernel in this process so far}"""
    return _info(load().sd_split_info, ("kmax", "lmax", "nmax", "launches"))


def split_rows(sym, R, K=64, min_size=8, max_iter=16, device=None, threads=1):
    """The subfamilies of the rows of a symbol matrix (csrc/sd_split.hpp; include/sd_hip.h: sd_split_*): sym = uint8 [n, L],
    0..4 = A C G T N, 5 = deleted; R the radius in columns, K the most subfamilies, min_size the fewest rows of a new one,
    max_iter the Lloyd iterations per round.  device=None: host threads (sd_split_host); else the kernels of
    csrc/sd_split.hip on that device (L > 512: the host form inside the call).  Both give the same integers.
    -> formats.Split"""
    import numpy as np
    from . import formats
    who = "split_rows"
    R, K, S, I = _split_args(R, K, min_size, max_iter, who)
    a = np.ascontiguousarray(sym, dtype=np.uint8)
    if a.ndim != 2 or a.shape[1] < 1:
        raise SdError(SD_ERR_PARAM, "%s: sym must be [n, L] with L >= 1" % who)
    n, L = int(a.shape[0]), int(a.shape[1])
    if n > SPLIT_NMAX:
        raise SdError(SD_ERR_PARAM, "%s: %d member rows, the cap is %d (SPLIT_NMAX)" % (who, n, SPLIT_NMAX))
    if n and int(a.max()) > 5:
        raise SdError(SD_ERR_PARAM, "%s: a symbol above 5 (0..4 = A C G T N, 5 = deleted)" % who)
    cen = np.zeros((K, L), dtype=np.uint8)
    asg, d1, d2 = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
    sizes = np.zeros(K, dtype=np.int32)
    info = (C.c_int64 * 4)()
    err = _err()
    L_ = load()
    base = a.ctypes.data if n else cen.ctypes.data
    if device is None:
        rc = L_.sd_split_host(base, n, L, L, R, K, S, I, int(threads), cen.ctypes.data, asg.ctypes.data, d1.ctypes.data, d2.ctypes.data,
                              sizes.ctypes.data, info, err, 1024)
    else:
        rc = L_.sd_split_dev(base, n, L, L, R, K, S, I, int(device), int(threads), cen.ctypes.data, asg.ctypes.data, d1.ctypes.data,
                             d2.ctypes.data, sizes.ctypes.data, info, err, 1024)
    _text_check(rc, err, "sd_split" + ("_host" if device is None else "_dev"))
    k = int(info[0])
    return formats.Split(cen[:k].copy(), asg[:n], d1[:n], d2[:n], sizes[:k].copy(), int(info[1]), int(info[2]))


def split_msa(msa, pair_tmpl, mono_lens, P, K=64, min_size=8, max_iter=16, device=None, threads=1):
    """The subfamilies of every forward monomer's instances in a host formats.Msa: per monomer m the rows of
    formats.split_members (status 1, either strand), radius split_radius(P, mono_lens[m]) -> [formats.Split], one per
    monomer (k = 0 for a monomer without instances)."""
    import numpy as np
    from . import formats
    _split_percent(P, "split_msa")
    _split_args(1, K, min_size, max_iter, "split_msa")
    groups = [[] for _ in mono_lens]
    for i, il in enumerate(pair_tmpl):
        if int(msa.status[i]) == 1:
            groups[int(il) >> 1].append(i)
    out = []
    for m, L in enumerate(mono_lens):
        L = int(L)
        sym = np.zeros((len(groups[m]), max(L, 1)), dtype=np.uint8)
        for x, i in enumerate(groups[m]):
            at = int(msa.row_at[i])
            sym[x, :L] = msa.rows[at:at + L]
        out.append(split_rows(sym, split_radius(P, L), K, min_size, max_iter, device=device, threads=threads))
    return out


class JobSplit(namedtuple("JobSplit", "sub d1 d2 centres cen_off sizes info")):
    """The subfamilies of all monomers of a job (final_split_host): sub / d1 / d2 = int32 [n_rows] (-1 for a row that is no
    member), centres = flat uint8, monomer m's k_m x L_m symbol bytes at centres[cen_off[m]:cen_off[m + 1]]; cen_off = int64
    [n_mono + 1], sizes = int32 [n_mono, K], info = int64 [n_mono, 4] = (member rows, k, rounds, Lloyd iterations)."""
    __slots__ = ()


def _split_job_args(mono_lens, P, K, min_size, max_iter, who):
    import numpy as np
    _split_percent(P, who)
    _, K, S, I = _split_args(1, K, min_size, max_iter, who)
    ml = np.ascontiguousarray(mono_lens, dtype=np.int32)
    if len(ml) and int(ml.min()) < 1:
        raise SdError(SD_ERR_PARAM, "%s: an empty monomer" % who)
    rad = np.ascontiguousarray([split_radius(P, x) for x in ml.tolist()], dtype=np.int32)
    return ml, rad, K, S, I


def final_split_host(msa, pair_tmpl, mono_lens, P, K=64, min_size=8, max_iter=16, threads=1):
    """All monomers of a job in one call, on host threads (sd_split_final_host): msa = a formats.Msa (final_msa_host, or
    DeviceMsa.to_host()), pair_tmpl = its interleaved templates -> JobSplit (numpy arrays)."""
    import numpy as np
    who = "final_split_host"
    ml, rad, K, S, I = _split_job_args(mono_lens, P, K, min_size, max_iter, who)
    n, M = len(pair_tmpl), len(ml)
    fmono = np.ascontiguousarray(np.asarray(pair_tmpl, dtype=np.int32).reshape(-1) >> 1)
    rows = np.ascontiguousarray(msa.rows, dtype=np.uint8)
    row_at = np.ascontiguousarray(msa.row_at, dtype=np.int64)
    status = np.ascontiguousarray(msa.status, dtype=np.uint8)
    cap = int(K) * int(ml.sum()) if M else 0
    sub, d1, d2 = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
    centres = np.zeros(max(cap, 1), dtype=np.uint8)
    cen_off = np.zeros(M + 1, dtype=np.int64)
    sizes = np.zeros((M, K), dtype=np.int32)
    info = np.zeros((M, 4), dtype=np.int64)
    err = _err()
    rc = load().sd_split_final_host(rows.ctypes.data, row_at.ctypes.data, status.ctypes.data, fmono.ctypes.data, n, ml.ctypes.data,
                                    rad.ctypes.data, M, K, S, I, int(threads), sub.ctypes.data, d1.ctypes.data, d2.ctypes.data,
                                    centres.ctypes.data, cap, cen_off.ctypes.data, sizes.ctypes.data, info.ctypes.data, err, 1024)
    _text_check(rc, err, "sd_split_final_host")
    return JobSplit(sub[:n], d1[:n], d2[:n], centres[:int(cen_off[-1])], cen_off, sizes, info)


def split_kernel_bench(sym, R, K=64, min_size=8, max_iter=16, device=0, warmup=2, reps=5):
    """sd_split_kernel_bench -> {"prep_ms", "assign_ms", "modes_ms": [...], "k", "rounds", "iters", "launches"}: the whole
    split once, then each stage timed on its final centres."""
    import numpy as np
    R, K, S, I = _split_args(R, K, min_size, max_iter, "split_kernel_bench")
    a = np.ascontiguousarray(sym, dtype=np.uint8)
    if a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= SPLIT_LMAX:
        raise SdError(SD_ERR_PARAM, "split_kernel_bench: sym must be [n, L] with n >= 1 and 1 <= L <= %d" % SPLIT_LMAX)
    return _bench(load().sd_split_kernel_bench, (a.ctypes.data, a.shape[0], a.shape[1], a.shape[1], R, K, S, I, int(device), int(warmup),
                                                 int(reps)), ("prep_ms", "assign_ms", "modes_ms"), ("k", "rounds", "iters", "launches"), reps)


HOR_MMAX = 2048
HOR_PMAX = 64
HOR_NAME_MAX = 192


def hor_unit_dtype():
    """numpy dtype of sd_hor_unit (include/sd_hip.h): first_row, start, end, mask, read, n_rows, order (0-based), strand
    (0 '+', 1 '-'); 48 bytes, no padding."""
    import numpy as np
    dt = np.dtype([("first_row", "<i8"), ("start", "<i8"), ("end", "<i8"), ("mask", "<u8"), ("read", "<i4"), ("n_rows", "<i4"),
                   ("order", "<i4"), ("strand", "<i4")])
    assert dt.itemsize == 48
    return dt


def hor_info():
    """sd_hor_info -> {"mmax": the most monomers, "pmax": the most monomers of an order and rows of a unit, "name_max": the
    bytes a name needs}"""
    return _info(load().sd_hor_info, ("mmax", "pmax", "name_max"), slots=4)


def hor_name(mask):
    """The name of a unit's mask: the positions present as ascending ranges joined by '_' (sd_hor_name)"""
    buf = C.create_string_buffer(HOR_NAME_MAX)
    load().sd_hor_name(int(mask) & 0xFFFFFFFFFFFFFFFF, buf)
    return buf.value.decode()


def _hor_args(n_mono, G, C_, who):
    """integers that fit the C types; the ranges are the library's to refuse, with its texts"""
    for name, v, bits in (("n_mono", n_mono, 31), ("G", G, 63), ("C", C_, 63)):
        _int_arg(who, name, v, -(1 << bits), (1 << bits) - 1, "")
    return n_mono, G, C_


class _HorOut:
    """the host arrays a sd_hor_* call fills, and the formats.Hor made of them"""

    def __init__(self, n, M):
        import numpy as np
        M1 = max(M, 1) if 0 < M <= HOR_MMAX else 1
        self.n, self.M = n, M1
        self.T = np.zeros((M1, M1), dtype=np.int64)
        self.rows = np.zeros(M1, dtype=np.int64)
        self.hor, self.pos, self.kind, self.len, self.lfirst, self.llen = (np.zeros(M1, dtype=np.int32) for _ in range(6))
        self.info = (C.c_int64 * 4)()
        self.err = _err()
        self.row_unit = np.zeros(max(n, 1), dtype=np.int32)
        self.units = np.zeros(max(n, 1), dtype=hor_unit_dtype())   # (n_rows always suffices)

    def orders(self):
        return [x.ctypes.data for x in (self.rows, self.hor, self.pos, self.kind, self.len, self.lfirst, self.llen)]

    def tail(self):
        return [self.T.ctypes.data] + self.orders() + [self.row_unit.ctypes.data, self.units.ctypes.data, self.n, self.info, self.err, 1024]

    def result(self):
        from . import formats
        no, nl = int(self.info[0]), int(self.info[2])
        return formats.Hor(self.T, self.rows, self.hor, self.pos, self.kind[:no].copy(), self.len[:no].copy(),
                           [(int(a), int(b)) for a, b in zip(self.lfirst[:nl], self.llen[:nl])], self.row_unit[:self.n],
                           self.units[:int(self.info[1])].copy())


def hor_rows(read, start, end, key, usable, n_mono, G=0, C_=2, threads=1, cap_units=None):
    """The higher-order repeat units of final rows given as columns (csrc/sd_hor.hpp; include/sd_hip.h: sd_hor_*): read,
    start, end (inclusive), key = 2 m + s (monomer m, s = 1 the reverse complement; -1: none), usable (reliable); n_mono
    monomers, G the widest gap adjacency bridges, C_ the fewest pairs behind an edge of an order.  Runs on host threads
    (sd_hor_rows).  cap_units: the units allocated (None: one per row, which always suffices; fewer than the job has is
    SD_ERR_PARAM with the count).  -> formats.Hor"""
    import numpy as np
    who = "hor_rows"
    M, G, C_ = _hor_args(n_mono, G, C_, who)
    cols = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((read, np.int32), (start, np.int64), (end, np.int64),
                                                                      (key, np.int32), (usable, np.uint8))]
    n = int(cols[0].shape[0])
    if any(int(a.shape[0]) != n for a in cols):
        raise SdError(SD_ERR_PARAM, "%s: the five columns differ in length" % who)
    o = _HorOut(n, M)
    ptrs = [a.ctypes.data if n else o.T.ctypes.data for a in cols]
    tail = o.tail()
    if cap_units is not None:
        tail[10] = min(int(cap_units), max(n, 1))
    _text_check(load().sd_hor_rows(*ptrs, n, M, G, C_, int(threads), *tail), o.err, "sd_hor_rows")
    return o.result()


def final_hor_host(final_rows, n_mono, G=0, C_=2, threads=1):
    """hor_rows on the rows of a final-mode job (sd_hor_final_host): final_rows = a FinalRows or its (rows, row_off, alt); key =
    best, usable = reliable == 1 -> formats.Hor"""
    import numpy as np
    M, G, C_ = _hor_args(n_mono, G, C_, "final_hor_host")
    rows = np.ascontiguousarray(final_rows[0])
    n = int(rows.shape[0])
    o = _HorOut(n, M)
    _text_check(load().sd_hor_final_host(rows.ctypes.data if n else o.T.ctypes.data, n, M, G, C_, int(threads), *o.tail()), o.err,
                "sd_hor_final_host")
    return o.result()


def decompose_files_records(reads_fa, monomers_fa, records_out, **kw):
    """reads.fa + monomers.fa -> binary record stream (sd_decompose_files_records): the rows of the raw TSV, no text."""
    L = load()
    p = make_params(**kw)
    err = C.create_string_buffer(4096)
    rc = L.sd_decompose_files_records(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p),
                                      os.fsencode(records_out), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def write_records(path, tmpl_names, read_names, read_lens, rows, row_off, **kw):
    """sd_write_records (host only): rows = structured array / sequence of (tmpl, start, end, score), row_off[n_reads + 1]."""
    import numpy as np
    L = load()
    p = make_params(**kw)
    r = np.ascontiguousarray(np.asarray(rows, dtype=_rec_dtype()) if not isinstance(rows, np.ndarray) else rows, dtype=_rec_dtype())
    o = np.ascontiguousarray(row_off, dtype=np.int64)
    rl = None if read_lens is None else np.ascontiguousarray(read_lens, dtype=np.int64)
    err = C.create_string_buffer(4096)
    rc = L.sd_write_records(os.fsencode(path), C.byref(p), _strs([_b(t) for t in tmpl_names]), len(tmpl_names),
                            _strs([_b(x) for x in read_names]), None if rl is None else rl.ctypes.data, len(read_names),
                            r.ctypes.data, o.ctypes.data, err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def read_records(path):
    """sd_read_records (host only) -> dict(params, templates, reads, read_lens, row_off, rows[structured array])."""
    import numpy as np
    L = load()
    out = Records()
    err = C.create_string_buffer(4096)
    rc = L.sd_read_records(os.fsencode(path), C.byref(out), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    try:
        n, nr = out.n_reads, out.n_rows
        res = {"params": {"scoring": (out.ins, out.del_, out.mismatch, out.match), "part_size": out.part_size,
                          "overlap": out.overlap, "ed_thr": out.ed_thr},
               "templates": [out.tmpl_names[t].decode() for t in range(out.n_templates)],
               "reads": [out.read_names[r].decode() for r in range(n)],
               "read_lens": [int(out.read_lens[r]) for r in range(n)],
               "row_off": np.ctypeslib.as_array(out.row_off, shape=(n + 1,)).copy(),
               "rows": (np.frombuffer(C.string_at(out.rows, nr * C.sizeof(Rec)), dtype=_rec_dtype()).copy() if nr
                        else np.zeros(0, dtype=_rec_dtype()))}
    finally:
        L.sd_records_free(C.byref(out))
    return res


def records_to_raw_tsv(records_path, raw_tsv_out, threads=1):
    """sd_records_to_raw_tsv (host only): the raw TSV `dp` prints for the rows of a record stream."""
    L = load()
    err = C.create_string_buffer(4096)
    rc = L.sd_records_to_raw_tsv(os.fsencode(records_path), os.fsencode(raw_tsv_out), int(threads), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def last_run_stats():
    """Stage times of the last run_files / run_files_range call of this process (sd_last_run_stats)."""
    L = load()
    v = (C.c_double * 24)()
    L.sd_last_run_stats(v)
    keys = ("fill_ms", "trace_ms", "compact_ms", "ident_ms", "ident_pairs", "batches", "rows", "pack_ms", "wait_ms",
            "raw_text_ms", "post_ms", "io_ms", "text_identity_ms", "final_text_ms", "total_ms", "alloc_ms", "setup_ms",
            "assemble_ms", "homo_pairs", "homo_full_pairs",
            # a screened job (run_files(screen=...)): the screen's wall and kernel time, bases read and decomposed
            "screen_ms", "screen_kernel_ms", "screen_bases_read", "screen_bases_decomposed")
    return dict(zip(keys, [float(x) for x in v]))


def last_run_device_stats():
    """Per device entry of the last run_files call of this process (sd_last_run_device_stats): a list of
    {"batches": batches dealt to the entry, "busy_ms": its device busy time (HIP-event spans of its batches)}."""
    L = load()
    b = (C.c_int64 * 16)()
    ms = (C.c_double * 16)()
    n = L.sd_last_run_device_stats(b, ms, 16)
    return [{"batches": int(b[i]), "busy_ms": float(ms[i])} for i in range(min(n, 16))]


def multi_device_selftest():
    """Host-only check of the batch dealing of run_files(devices=...) (sd_multi_device_selftest); raises on a
    broken property."""
    L = load()
    err = C.create_string_buffer(1024)
    rc = L.sd_multi_device_selftest(err, 1024)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def run_files_range(reads_fa, monomers_fa, rank, world, raw_tsv_out, final_tsv_out, alt_tsv_out, min_identity=0,
                    second_best=False, lr_coef=(-31.48494996, 0.41784018, 0.69186882), **kw):
    """One rank's group of reads of a multi-process launch, completely (sd_run_files_range) -> (first read, one
    past the last read, reads in the file, chunks of this rank).  SdError(SD_ERR_UNSUPPORTED) when the read set
    cannot be split by reads."""
    L = load()
    p = make_params(**kw)
    err = C.create_string_buffer(4096)
    coef = (C.c_double * 3)(*[float(x) for x in lr_coef])
    info = (C.c_int64 * 4)()
    rc = L.sd_run_files_range(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), int(rank), int(world),
                              os.fsencode(raw_tsv_out), os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out),
                              int(min_identity), 1 if second_best else 0, coef, info, err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    return tuple(info)


def convert_raw_tsv(raw_tsv, reads_fa, monomers_fa, final_tsv_out, alt_tsv_out, min_identity=0, second_best=False,
                    lr_coef=(-31.48494996, 0.41784018, 0.69186882), device=-1, threads=1):
    """convert_tsv (main.py:168-184) natively; device=-1: host identities, else the HIP kernel."""
    L = load()
    err = C.create_string_buffer(4096)
    coef = (C.c_double * 3)(*[float(x) for x in lr_coef])
    rc = L.sd_convert_raw_tsv(os.fsencode(raw_tsv), os.fsencode(reads_fa), os.fsencode(monomers_fa),
                              os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out), int(min_identity),
                              1 if second_best else 0, coef, int(device), int(threads), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def convert_raw_tsv_range(raw_tsv, reads_fa, monomers_fa, final_tsv_out, alt_tsv_out, rank, world, min_identity=0,
                          second_best=False, lr_coef=(-31.48494996, 0.41784018, 0.69186882), device=-1, threads=1):
    """convert_tsv on this rank's byte range of the raw TSV (cut at line starts) into this rank's part files."""
    L = load()
    err = C.create_string_buffer(4096)
    coef = (C.c_double * 3)(*[float(x) for x in lr_coef])
    rc = L.sd_convert_raw_tsv_range(os.fsencode(raw_tsv), os.fsencode(reads_fa), os.fsencode(monomers_fa),
                                    os.fsencode(final_tsv_out), os.fsencode(alt_tsv_out), int(min_identity),
                                    1 if second_best else 0, coef, int(device), int(threads), int(rank), int(world), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def decompose(read_names, read_seqs, mono_names, mono_seqs, **kw):
    """In-memory variant -> raw TSV bytes."""
    L = load()
    p = make_params(**kw)
    err = C.create_string_buffer(4096)
    rs = [_b(s) for s in read_seqs]
    ms = [_b(s) for s in mono_seqs]
    rl = (C.c_int64 * max(len(rs), 1))(*[len(s) for s in rs])
    ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
    out = C.c_void_p()
    ln = C.c_size_t()
    rc = L.sd_decompose(_strs(read_names), _strs(rs), rl, len(rs), None if mono_names is None else _strs(mono_names), _strs(ms), ml,
                        len(ms), C.byref(p), C.byref(out), C.byref(ln), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    data = C.string_at(out, ln.value)
    L.sd_free(out)
    return data


class Engine:
    """Device-resident batches: create (templates) -> load_reads -> run -> fetch -> assemble."""

    def __init__(self, mono_seqs, **kw):
        self.L = load()
        self.params = make_params(**kw)
        self._err = C.create_string_buffer(4096)
        ms = [_b(s) for s in mono_seqs]
        ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
        self.h = C.c_void_p()
        rc = self.L.sd_engine_create(C.byref(self.h), C.byref(self.params), _strs(ms), ml, len(ms),
                                     self._err, 4096)
        self._check(rc)
        self.n_chunks = 0
        self.n_reads = 0

    def _check(self, rc):
        if rc != SD_OK:
            raise SdError(rc, self._err.value.decode(errors="replace"))

    def close(self):
        if self.h:
            self.L.sd_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_reads(self, read_seqs):
        """Loads a batch: a list of sequences (packed on the host), or a DeviceReads (packed on the device)."""
        if isinstance(read_seqs, DeviceReads):
            d = read_seqs
            self._keep = d
            n = C.c_int64()
            self._check(self.L.sd_engine_load_reads_dev(self.h, C.c_void_p(d.ptr), d.c_off, d.c_lens, d.n,
                                                        C.c_void_p(d.stream), C.byref(n), self._err, 4096))
            self.n_chunks = n.value
            self.n_reads = d.n
            return n.value
        rs = [_b(s) for s in read_seqs]
        self._keep = rs
        rl = (C.c_int64 * max(len(rs), 1))(*[len(s) for s in rs])
        n = C.c_int64()
        self._check(self.L.sd_engine_load_reads(self.h, _strs(rs), rl, len(rs), C.byref(n), self._err, 4096))
        self.n_chunks = n.value
        self.n_reads = len(rs)
        return n.value

    def run(self, stream=None):
        self._check(self.L.sd_engine_run(self.h, C.c_void_p(stream or 0), self._err, 4096))

    def fetch_raw(self):
        recs = C.POINTER(Rec)()
        off = C.POINTER(C.c_int64)()
        self._check(self.L.sd_engine_fetch(self.h, C.byref(recs), C.byref(off), self._err, 4096))
        return recs, off

    def fetch(self):
        """-> list over chunks of [(tmpl, start, end, score), ...] (chunk-local coordinates)."""
        recs, off = self.fetch_raw()
        out = []
        for c in range(self.n_chunks):
            out.append([(recs[x].tmpl, recs[x].start, recs[x].end, recs[x].score)
                        for x in range(off[c], off[c + 1])])
        self.L.sd_free(recs)
        self.L.sd_free(off)
        return out

    def rows(self):
        """run results assembled per read -> list over reads of [(tmpl, start, end, score), ...]."""
        recs, off = self.fetch_raw()
        rows = C.POINTER(Rec)()
        roff = C.POINTER(C.c_int64)()
        self._check(self.L.sd_engine_assemble(self.h, recs, off, C.byref(rows), C.byref(roff), self._err, 4096))
        out = []
        for r in range(self.n_reads):
            out.append([(rows[x].tmpl, rows[x].start, rows[x].end, rows[x].score)
                        for x in range(roff[r], roff[r + 1])])
        for p in (recs, off, rows, roff):
            self.L.sd_free(p)
        return out

    def rows_device(self, stream=None):
        """The rows of the run assembled on the DEVICE (sd_engine_rows_dev) -> DeviceRows, what rows() returns as
        lists; ordered on `stream` as Stream.collect_device."""
        import torch
        dev = torch.device("cuda", self.params.device)
        st = _torch_stream(torch, dev, stream)
        with torch.cuda.stream(st):
            row_off = torch.empty(self.n_reads + 1, dtype=torch.int64, device=dev)
        # the first call assembles and, without room, only reports the exact row count (no record crosses to the
        # host); the second copies into a tensor of that size
        n = C.c_int64()
        rc = self.L.sd_engine_rows_dev(self.h, None, 0, C.c_void_p(row_off.data_ptr()), C.c_void_p(st.cuda_stream),
                                       C.byref(n), self._err, 4096)
        if rc != SD_ERR_PARAM or n.value <= 0:
            self._check(rc)
        with torch.cuda.stream(st):
            rows = torch.empty((max(n.value, 1), 4), dtype=torch.int32, device=dev)
        if n.value > 0:
            self._check(self.L.sd_engine_rows_dev(self.h, C.c_void_p(rows.data_ptr()), n.value, C.c_void_p(row_off.data_ptr()),
                                                  C.c_void_p(st.cuda_stream), C.byref(n), self._err, 4096))
        return DeviceRows(rows[:n.value], row_off, int(n.value))

    def total_rows(self):
        """Number of assembled rows (cheap check used by bench.py)."""
        recs, off = self.fetch_raw()
        n = off[self.n_chunks]
        self.L.sd_free(recs)
        self.L.sd_free(off)
        return n

    def timings(self):
        ms = (C.c_float * 4)()
        rc = self.L.sd_engine_timings(self.h, ms)
        if rc != SD_OK:
            raise SdError(rc, "sd_engine_timings")
        return {"fill_ms": ms[0], "trace_ms": ms[1], "compact_ms": ms[2], "run_ms": ms[3]}

    def info(self):
        v = (C.c_int64 * 8)()
        self.L.sd_engine_info(self.h, v)
        return _info_dict(v)

    def filter_result(self):
        """The --ed_thr prefilter's result of the fetched batch (sd_engine_filter_result, for tests) -> (dist, rank):
        int32 / uint16 arrays [n_chunks, T]; rank = place in the chunk's filtered order, 0xffff = dropped."""
        import numpy as np
        T = int(self.info()["n_templates"])
        dist = np.empty((self.n_chunks, T), dtype=np.int32)
        rank = np.empty((self.n_chunks, T), dtype=np.uint16)
        n, t = C.c_int64(), C.c_int32()
        self._check(self.L.sd_engine_filter_result(self.h, dist.ctypes.data, rank.ctypes.data, dist.size, C.byref(n),
                                                   C.byref(t), self._err, 4096))
        if (n.value, t.value) != dist.shape:
            raise SdError(SD_ERR_INTERNAL, "filter_result: %d x %d, expected %d x %d" % ((n.value, t.value) + dist.shape))
        return dist, rank


def _info_dict(v):
    return {"n_templates": v[0], "sum_template_len": v[1], "n_chunks": v[2], "rows": v[3],
            "family": {1: "generic", 2: "fast"}.get(v[4] & 0xff, "?"),
            "cells": {0: "int32", 1: "int16", 2: "f16", 9: "u16", 3: "int16/int8-table", 4: "f16/bf8-table",
                      5: "f16/bf8-codes x waves", 6: "f16/bf8-codes tiled x waves", 7: "int16/int8-codes x waves",
                      8: "int16/int8-codes tiled x waves"}.get(v[4] >> 8, "?"),
            "cells_per_lane": v[5] if (v[4] & 0xff) == 1 else v[5] & 0xffff,
            "floor_slots": 0 if (v[4] & 0xff) == 1 else v[5] >> 16,
            "workspace_bytes": v[6], "fill_launches": v[7] & 0xffff,
            "trace": {0: "generic", 1: "one-block int32", 2: "two-block packed16"}.get(v[7] >> 16, "?")}


class ReadSet:
    """Sequences in host memory, as C arrays (built once, reusable across submits)."""

    def __init__(self, read_seqs):
        self.seqs = [_b(s) for s in read_seqs]
        self.n = len(self.seqs)
        self.ptrs = _strs(self.seqs)
        self.lens = (C.c_int64 * max(self.n, 1))(*[len(s) for s in self.seqs])
        self.bp = sum(len(s) for s in self.seqs)


def _device_buffer(data, stream):
    """(ptr, nbytes, device, stream, shape, strides) of `data`: a (ptr, nbytes, device) tuple, or anything with the
    tensor interface of torch (data_ptr / is_cuda / dtype / shape / stride / device) -- torch itself is not imported
    here.  stream=None with a tensor: the current stream of the tensor's device, as the tensor's own module gives it."""
    if isinstance(data, tuple):
        if len(data) != 3:
            raise SdError(SD_ERR_PARAM, "device reads: the tuple form is (ptr, nbytes, device)")
        ptr, nbytes, device = (int(x) for x in data)
        return ptr, nbytes, device, int(stream or 0), (nbytes,), (1,)
    if not hasattr(data, "data_ptr"):
        raise SdError(SD_ERR_PARAM, "device reads: a tensor on a HIP device or a (ptr, nbytes, device) tuple")
    if not str(data.dtype).endswith("uint8"):
        raise SdError(SD_ERR_PARAM, "device reads: the tensor must be uint8, not %s" % data.dtype)
    if not getattr(data, "is_cuda", False):
        raise SdError(SD_ERR_PARAM, "device reads: the tensor must lie on a HIP device (a CPU tensor goes in as a read list)")
    shape = tuple(int(x) for x in data.shape)
    strides = tuple(int(x) for x in data.stride())
    if len(shape) not in (1, 2):
        raise SdError(SD_ERR_PARAM, "device reads: a 1-D tensor of concatenated reads or a 2-D [n, width] tensor of padded rows")
    if shape[-1] > 1 and strides[-1] != 1:
        raise SdError(SD_ERR_PARAM, "device reads: the last dimension must be contiguous")
    if len(shape) == 2 and shape[0] > 1 and strides[0] < 0:
        raise SdError(SD_ERR_PARAM, "device reads: negative row stride")
    nbytes = shape[0] if len(shape) == 1 else ((shape[0] - 1) * strides[0] + shape[1] if shape[0] > 0 else 0)
    device = getattr(data.device, "index", None) or 0
    if stream is None:
        import sys
        mod = sys.modules.get(type(data).__module__.split(".")[0])
        cur = getattr(getattr(mod, "cuda", None), "current_stream", None)
        stream = cur(device).cuda_stream if cur is not None else 0
    return int(data.data_ptr()), int(nbytes), int(device), int(stream or 0), shape, strides


DeviceRows = namedtuple("DeviceRows", "rows row_off n_rows")
"""Rows that stay in device memory (Stream.collect_device, Engine.rows_device): rows = an int32 [n_rows, 4] torch tensor
(tmpl, start, end, score per row: the layout of sd_rec), row_off = int64 [n_reads + 1] on the same device (read r owns
rows[row_off[r]:row_off[r+1]]), n_rows as a Python int."""


class DeviceFinalRows(namedtuple("DeviceFinalRows", "rows row_off alt n_rows")):
    """Final rows that stay in device memory (Stream.collect_final_device): rows = a uint8 [n_rows, 80] torch tensor (the
    bytes of sd_final_row: on the host it views as final_dtype()), row_off = int64 [n_reads + 1] on the same device, alt =
    float64 [n_rows, n_keys] (second_best) or None, n_rows as a Python int."""
    __slots__ = ()

    def to_host(self):
        """-> FinalRows (numpy), what Stream(final=True).collect() returns for the same job."""
        import numpy as np
        r = np.ascontiguousarray(self.rows.cpu().numpy()).reshape(-1).view(final_dtype())
        return FinalRows(r, self.row_off.cpu().numpy(), None if self.alt is None else self.alt.cpu().numpy())


class DeviceProfile(namedtuple("DeviceProfile", "counts offsets names seqs")):
    """A profile that stays in device memory (Stream.profile_device): counts = a flat int64 torch tensor on the stream's
    device, monomer m's [L + 1, 12] block at counts[offsets[m]:offsets[m + 1]] (formats.PROFILE_COLUMNS; offsets, names
    and seqs are host lists)."""
    __slots__ = ()

    def to_host(self):
        """-> formats.Profile, what Stream.profile() returns for the same jobs."""
        from . import formats
        return formats.profile_from_counts(self.names, self.seqs, self.counts.cpu().numpy())


class DeviceText(namedtuple("DeviceText", "text row_pos read_pos")):
    """TSV text that stays in device memory (format_final_device / format_raw_device): text = a uint8 torch tensor of
    exactly the text's length, row_pos = int64 [n_rows + 1] (where the text of row i begins; for the _alt text: where the
    n_keys lines of final row i begin), read_pos = int64 [n_reads + 1] (where the text of read r begins), all on the rows'
    device."""
    __slots__ = ()

    def to_bytes(self):
        """The text copied to the host."""
        return self.text.cpu().numpy().tobytes()


class TextTables:
    """The name tables of the text calls (sd_text_tables): the read names of a job in submit order and the column
    names -- Stream.keys() for final rows, the DP's template names (monomers, then monomers + "'") for raw rows.  Uploaded
    to the device by the first format_*_device call that uses them and reused by later ones; close() waits for the last
    of those calls' kernels."""

    def __init__(self, read_names, col_names):
        self.L = load()
        self.n_reads, self.n_cols = len(read_names), len(col_names)
        self.h = C.c_void_p()
        err = _err()
        _text_check(self.L.sd_text_tables_create(C.byref(self.h), _strs(read_names), self.n_reads, _strs(col_names), self.n_cols,
                                                 err, 1024), err)

    def close(self):
        if self.h:
            self.L.sd_text_tables_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _text_tables(tables, read_names, col_names):
    """(tables, own): the caller's, or fresh ones this call closes"""
    if tables is not None:
        if tables.n_reads != len(read_names) or tables.n_cols != len(col_names):
            raise SdError(SD_ERR_PARAM, "tables: %d reads and %d columns, the call has %d and %d"
                          % (tables.n_reads, tables.n_cols, len(read_names), len(col_names)))
        return tables, False
    return TextTables(read_names, col_names), True


def format_final_device(dfr, read_names, keys, stream=None, tables=None):
    """The text of final_decomposition.tsv / _alt.tsv of a DeviceFinalRows, formatted on its device (sd_text_final_size_dev
    / sd_text_final_write_dev) -> (final, alt): DeviceText, alt None for rows without second_best.  read_names: the job's
    reads in submit order; keys: Stream.keys(); tables: a TextTables over the same names, to upload them once for many
    jobs.  torch allocates the tensors on `stream` (Stream.collect_final_device's convention) and the library fills them
    there: the host waits for the text's size only, and work enqueued on the stream afterwards sees the text."""
    L = load()
    torch, dev, st = _device_frame(dfr.row_off.device, stream)
    n, nr, nk = int(dfr.n_rows), len(read_names), len(keys)
    if dfr.row_off.shape[0] != nr + 1:
        raise SdError(SD_ERR_PARAM, "format_final_device: %d read names for %d reads" % (nr, dfr.row_off.shape[0] - 1))
    has_alt = dfr.alt is not None
    t, own = _text_tables(tables, read_names, keys)
    err = _err()
    try:
        with torch.cuda.stream(st):
            row_pos = torch.empty(n + 1, dtype=torch.int64, device=dev)
            read_pos = torch.empty(nr + 1, dtype=torch.int64, device=dev)
            alt_pos = torch.empty(n + 1, dtype=torch.int64, device=dev) if has_alt else None
            alt_read_pos = torch.empty(nr + 1, dtype=torch.int64, device=dev) if has_alt else None
        # (an empty alt still means "with _alt text": a pointer that is not NULL)
        alt_ptr = C.c_void_p((dfr.alt.data_ptr() if n and nk else alt_pos.data_ptr()) if has_alt else 0)
        fb, ab = C.c_int64(), C.c_int64()
        _text_check(L.sd_text_final_size_dev(t.h, _dptr(dfr.rows), n, _dptr(dfr.row_off), alt_ptr, nk, dev.index or 0,
                                             C.c_void_p(st.cuda_stream), _dptr(row_pos), _dptr(alt_pos), _dptr(read_pos),
                                             _dptr(alt_read_pos), C.byref(fb), C.byref(ab), err, 1024), err)
        with torch.cuda.stream(st):
            ftext = torch.empty(fb.value, dtype=torch.uint8, device=dev)
            atext = torch.empty(ab.value, dtype=torch.uint8, device=dev) if has_alt else None
        _text_check(L.sd_text_final_write_dev(t.h, _dptr(dfr.rows), n, alt_ptr, nk, dev.index or 0, C.c_void_p(st.cuda_stream),
                                              _dptr(row_pos), _dptr(alt_pos), _dptr(ftext), fb.value, _dptr(atext), ab.value, err, 1024),
                    err)
    finally:
        if own:
            t.close()
    return DeviceText(ftext, row_pos, read_pos), (DeviceText(atext, alt_pos, alt_read_pos) if has_alt else None)


def format_raw_device(drows, read_names, tmpl_names, stream=None, tables=None):
    """The text of _raw.tsv of a DeviceRows, formatted on its device (sd_text_raw_size_dev / sd_text_raw_write_dev) ->
    DeviceText.  tmpl_names: the DP's templates (monomers, then monomers + "'"); the rest as format_final_device."""
    L = load()
    torch, dev, st = _device_frame(drows.row_off.device, stream)
    n, nr = int(drows.n_rows), len(read_names)
    if drows.row_off.shape[0] != nr + 1:
        raise SdError(SD_ERR_PARAM, "format_raw_device: %d read names for %d reads" % (nr, drows.row_off.shape[0] - 1))
    t, own = _text_tables(tables, read_names, tmpl_names)
    err = _err()
    try:
        with torch.cuda.stream(st):
            row_pos = torch.empty(n + 1, dtype=torch.int64, device=dev)
            read_pos = torch.empty(nr + 1, dtype=torch.int64, device=dev)
            row_read = torch.empty(n, dtype=torch.int32, device=dev)
        nb = C.c_int64()
        _text_check(L.sd_text_raw_size_dev(t.h, _dptr(drows.rows), n, _dptr(drows.row_off), dev.index or 0, C.c_void_p(st.cuda_stream),
                                           _dptr(row_read), _dptr(row_pos), _dptr(read_pos), C.byref(nb), err, 1024), err)
        with torch.cuda.stream(st):
            text = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        _text_check(L.sd_text_raw_write_dev(t.h, _dptr(drows.rows), n, _dptr(drows.row_off), dev.index or 0, C.c_void_p(st.cuda_stream),
                                            _dptr(row_read), _dptr(row_pos), _dptr(text), nb.value, err, 1024), err)
    finally:
        if own:
            t.close()
    return DeviceText(text, row_pos, read_pos)


def _take_text(L, p, n):
    out = C.string_at(p, n.value) if p.value and n.value else b""
    L.sd_free(p)
    return out


def format_final_host(final_rows, read_names, keys, threads=1, positions=False):
    """The host twin of format_final_device (sd_text_final_host: the same source text, compiled for the host) on a
    FinalRows or its (rows, row_off, alt) -> (final bytes, alt bytes or None).  positions=True: ((bytes, row_pos,
    read_pos), (bytes, alt_pos, alt_read_pos) or None), the arrays of a DeviceText as numpy."""
    import numpy as np
    L = load()
    rows, row_off, alt = final_rows
    rows = np.ascontiguousarray(rows, dtype=final_dtype())
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    n, nr, nk = len(rows), len(read_names), len(keys)
    if len(row_off) != nr + 1:
        raise SdError(SD_ERR_PARAM, "format_final_host: %d read names for %d reads" % (nr, len(row_off) - 1))
    if alt is not None:
        alt = np.ascontiguousarray(alt, dtype=np.float64).reshape(-1)
        if len(alt) != n * nk:
            raise SdError(SD_ERR_PARAM, "format_final_host: alt is not n_rows x n_keys")
        alt = np.concatenate([alt, np.zeros(1)])   # (never NULL, also without rows)
    pos = [np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64), np.zeros(nr + 1, dtype=np.int64),
           np.zeros(nr + 1, dtype=np.int64)]
    t = TextTables(read_names, keys)
    err = C.create_string_buffer(1024)
    ft, at, fb, ab = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
    try:
        rc = L.sd_text_final_host(t.h, rows.ctypes.data, n, row_off.ctypes.data, None if alt is None else alt.ctypes.data, nk,
                                  int(threads), C.byref(ft), C.byref(fb), C.byref(at), C.byref(ab), pos[0].ctypes.data,
                                  pos[1].ctypes.data, pos[2].ctypes.data, pos[3].ctypes.data, err, 1024)
        _text_check(rc, err)
        ftext, atext = _take_text(L, ft, fb), _take_text(L, at, ab)
    finally:
        t.close()
    if positions:
        return (ftext, pos[0], pos[2]), (None if alt is None else (atext, pos[1], pos[3]))
    return ftext, (None if alt is None else atext)


def format_raw_host(rows, row_off, read_names, tmpl_names, threads=1, positions=False):
    """The host twin of format_raw_device (sd_text_raw_host) on rows ([n, 4] int32: tmpl, start, end, score, or a
    structured sd_rec array) and row_off -> bytes; positions=True: (bytes, row_pos, read_pos)."""
    import numpy as np
    L = load()
    rows = np.ascontiguousarray(rows)
    if rows.dtype != _rec_dtype():
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    n, nr = len(rows), len(read_names)
    if len(row_off) != nr + 1:
        raise SdError(SD_ERR_PARAM, "format_raw_host: %d read names for %d reads" % (nr, len(row_off) - 1))
    row_pos, read_pos = np.zeros(n + 1, dtype=np.int64), np.zeros(nr + 1, dtype=np.int64)
    t = TextTables(read_names, tmpl_names)
    err = C.create_string_buffer(1024)
    tx, nb = C.c_void_p(), C.c_int64()
    try:
        rc = L.sd_text_raw_host(t.h, rows.ctypes.data if n else None, n, row_off.ctypes.data, int(threads), C.byref(tx),
                                C.byref(nb), row_pos.ctypes.data, read_pos.ctypes.data, err, 1024)
        _text_check(rc, err)
        text = _take_text(L, tx, nb)
    finally:
        t.close()
    return (text, row_pos, read_pos) if positions else text


def _torch_stream(torch, dev, stream):
    """stream=None: the current stream of the device (DeviceReads' convention); an int: that hipStream_t; else a
    torch stream."""
    if stream is None:
        return torch.cuda.current_stream(dev)
    if isinstance(stream, int):
        return torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
    return stream


class DeviceReads:
    """Reads that already lie in device memory (sd_stream_submit_dev / sd_engine_load_reads_dev): Stream.submit,
    Stream.imap and Engine.load_reads take one wherever they take a read list or a ReadSet, and the bases are packed by
    a HIP kernel instead of host threads.

    data: a 1-D uint8 tensor on a HIP device (the reads back to back; offsets default to the running sum of lens), a
    2-D [n, width] uint8 tensor of padded rows (offsets default to i * row stride), or a (ptr, nbytes, device) tuple.
    lens: the read lengths; offsets: where each read starts, in bytes from the start of data (any order, gaps allowed).
    stream: the hipStream_t (an int) on which the bytes were produced; None = the tensor's device's current stream at
    this moment (0, the null stream, for the tuple form).  The library orders itself behind that stream and makes the
    stream wait for its last read of the buffer (sd_hip.h), so the tensor may be overwritten or freed on that stream
    right after a submit returns.  The object keeps a reference to data.

    lenient=True: the reads are normalised on `stream` by sd_normalize_dev (lower case folded, IUPAC ambiguity codes ->
    N) before anything else uses them.  For a tensor the normalised text goes into a new tensor that this object owns
    (self.data; the caller's bytes stay untouched); inplace=True normalises the caller's buffer instead, and is required
    for the tuple form (SdError(SD_ERR_PARAM) otherwise).  self.norm_stats: a 4 x int64 device tensor with the counters
    of sd_normalize_dev (tensor form only).  A byte the rule leaves alone still fails the stream with SD_ERR_SYMBOL."""

    def __init__(self, data, lens, offsets=None, stream=None, lenient=False, inplace=False):
        self.ptr, self.nbytes, self.device, self.stream, shape, strides = _device_buffer(data, stream)
        self.data = data
        self.norm_stats = None
        if lenient and isinstance(data, tuple) and not inplace:
            raise SdError(SD_ERR_PARAM, "device reads: lenient=True on a (ptr, nbytes, device) tuple needs inplace=True "
                                        "(the library owns no memory to put the normalised text in)")
        self.read_lens = [int(x) for x in lens]
        self.n = len(self.read_lens)
        if len(shape) == 2:
            if offsets is None and self.n > shape[0]:
                raise SdError(SD_ERR_PARAM, "device reads: %d lengths for %d rows" % (self.n, shape[0]))
            for i, ln in enumerate(self.read_lens):
                if ln > shape[1]:
                    raise SdError(SD_ERR_PARAM, "device reads: read %d is longer (%d) than a row (%d)" % (i, ln, shape[1]))
        if offsets is None:
            if len(shape) == 2:
                self.read_off = [i * strides[0] for i in range(self.n)]
            else:
                self.read_off, at = [], 0
                for ln in self.read_lens:
                    self.read_off.append(at)
                    at += ln
        else:
            self.read_off = [int(x) for x in offsets]
            if len(self.read_off) != self.n:
                raise SdError(SD_ERR_PARAM, "device reads: %d offsets for %d lengths" % (len(self.read_off), self.n))
        for i, (o, ln) in enumerate(zip(self.read_off, self.read_lens)):
            if o < 0 or ln < 0 or o + ln > self.nbytes:
                raise SdError(SD_ERR_PARAM, "device reads: read %d (offset %d, length %d) runs past the buffer (%d bytes)"
                              % (i, o, ln, self.nbytes))
        if self.n and not self.ptr:
            raise SdError(SD_ERR_PARAM, "device reads: null device pointer")
        self.c_off = (C.c_int64 * max(self.n, 1))(*self.read_off)
        self.c_lens = (C.c_int64 * max(self.n, 1))(*self.read_lens)
        self.bp = sum(self.read_lens)
        if lenient and self.n:
            self._normalize(inplace)

    def _normalize(self, inplace):
        dst, stats = self.ptr, None
        if not isinstance(self.data, tuple):
            import torch
            dev = torch.device("cuda", self.device)
            with torch.cuda.stream(_torch_stream(torch, dev, self.stream)):   # (the blocks belong to the reads' stream)
                self.norm_stats = torch.zeros(4, dtype=torch.int64, device=dev)
                if not inplace:
                    own = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
                    dst = int(own.data_ptr())
            stats = C.c_void_p(int(self.norm_stats.data_ptr()))
        err = C.create_string_buffer(4096)
        rc = load().sd_normalize_dev(C.c_void_p(self.ptr), C.c_void_p(dst), self.c_off, self.c_lens, self.n, self.device,
                                     C.c_void_p(self.stream), stats, err, 4096)
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        if dst != self.ptr:
            self.ptr, self.data = dst, own


def normalize_host(data, inplace=False):
    """The lenient rule on host bytes (sd_normalize_host) -> (bytes, stats): stats = [lower-case bytes folded, ambiguity
    codes turned into N, bytes still outside ACGTN, bytes examined].  inplace=True: data is a writable buffer (bytearray,
    numpy uint8 array) that is normalised where it lies and returned."""
    L = load()
    stats = (C.c_uint64 * 4)()
    if inplace:
        mv = memoryview(data).cast("B")
        n = len(mv)
        buf = (C.c_char * n).from_buffer(data) if n else None
        rc = L.sd_normalize_host(buf and C.addressof(buf), buf and C.addressof(buf), n, stats)
        out = data
    else:
        src = bytes(data)
        n = len(src)
        dst = C.create_string_buffer(max(n, 1))
        rc = L.sd_normalize_host(C.cast(C.c_char_p(src), C.c_void_p), C.addressof(dst), n, stats)
        out = dst.raw[:n]
    if rc != SD_OK:
        raise SdError(rc, "sd_normalize_host")
    return out, [int(x) for x in stats]


def normalize_device(data, lens, offsets=None, out=None, stream=None, stats=None):
    """The lenient rule on reads in device memory (sd_normalize_dev): data, lens, offsets and stream as for DeviceReads
    (or data = a DeviceReads); out = None normalises in place, else a buffer of the same form that takes the reads at
    the same offsets; stats = a 4 x int64 / uint64 device tensor (or device address) the counters are added to.  The
    kernel is enqueued on the stream; nothing waits."""
    L = load()
    dr = data if isinstance(data, DeviceReads) else DeviceReads(data, lens, offsets=offsets, stream=stream)
    st = dr.stream if stream is None else (stream if isinstance(stream, int) else int(stream.cuda_stream))
    dst = dr.ptr
    if out is not None:
        dst, nb, dev, _, _, _ = _device_buffer(out, st)
        if nb < max([o + n for o, n in zip(dr.read_off, dr.read_lens)] or [0]):
            raise SdError(SD_ERR_PARAM, "normalize_device: the output buffer is shorter than the reads reach")
    sp = None if stats is None else C.c_void_p(int(stats.data_ptr()) if hasattr(stats, "data_ptr") else int(stats))
    err = C.create_string_buffer(4096)
    rc = L.sd_normalize_dev(C.c_void_p(dr.ptr), C.c_void_p(dst), dr.c_off, dr.c_lens, dr.n, dr.device, C.c_void_p(st), sp,
                            err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


def pack_bases_device(data, chunk_off, chunk_len, stream=None, fill=0):
    """The device packer alone (sd_pack_bases_dev): chunk c = data[chunk_off[c] : chunk_off[c] + chunk_len[c]], data as
    for DeviceReads (or a DeviceReads).  -> (bases2, nmask, has_n, first_bad): the chunks' 2-bit words back to back,
    their mask words back to back ((len + 31) // 32 each, written only for chunks that hold an N: the others keep
    `fill`), has_n per chunk, and the smallest offset of a byte outside ACGTN or -1."""
    import numpy as np
    L = load()
    if isinstance(data, DeviceReads):
        ptr, nbytes, device, st = data.ptr, data.nbytes, data.device, data.stream if stream is None else int(stream)
    else:
        ptr, nbytes, device, st, _, _ = _device_buffer(data, stream)
    off = np.ascontiguousarray(chunk_off, dtype=np.int64)
    ln = np.ascontiguousarray(chunk_len, dtype=np.int32)
    if off.shape != ln.shape or off.ndim != 1:
        raise SdError(SD_ERR_PARAM, "pack_bases_device: chunk_off and chunk_len differ in length")
    if len(off) and (off.min() < 0 or ln.min() <= 0 or int((off + ln).max()) > nbytes):
        raise SdError(SD_ERR_PARAM, "pack_bases_device: a chunk runs past the buffer")
    w = np.full(int(((ln.astype(np.int64) + 15) // 16).sum()), fill, dtype=np.uint32)
    m = np.full(int(((ln.astype(np.int64) + 31) // 32).sum()), fill, dtype=np.uint32)
    hn = np.zeros(max(len(ln), 1), dtype=np.int32)
    bad = C.c_int64(-1)
    rc = L.sd_pack_bases_dev(C.c_void_p(ptr), off.ctypes.data, ln.ctypes.data, len(ln), device, C.c_void_p(st),
                             w.ctypes.data, m.ctypes.data, hn.ctypes.data, C.byref(bad))
    if rc != SD_OK:
        raise SdError(rc, "sd_pack_bases_dev")
    return w, m, hn[:len(ln)], int(bad.value)


def final_dtype():
    """numpy dtype of sd_final_row (include/sd_hip.h): read, start, end, best, second, homo_best, homo_second (key
    indices into Stream.keys(), -1 = None), ident, second_ident, homo_ident, homo_second_ident, reliable."""
    import numpy as np
    dt = np.dtype([("read", "<i4"), ("start", "<i8"), ("end", "<i8"), ("best", "<i4"), ("second", "<i4"),
                   ("homo_best", "<i4"), ("homo_second", "<i4"), ("ident", "<f8"), ("second_ident", "<f8"),
                   ("homo_ident", "<f8"), ("homo_second_ident", "<f8"), ("reliable", "i1")], align=True)
    assert dt.itemsize == C.sizeof(FinalRec)
    return dt


FinalRows = namedtuple("FinalRows", "rows row_off alt")
"""A final-mode job: rows (numpy, final_dtype()), row_off (n_reads + 1: read r owns rows[row_off[r]:row_off[r+1]]) and
alt (n_rows x n_keys identities in key order, second_best only, else None)."""


class Stream:
    """Pipelined sequences-in-host-memory -> rows-in-host-memory path (sd_stream_*): submit() read sets,
    collect() their rows in FIFO order; two device batches are in flight across job boundaries.

    final=True (sd_stream_create_final): collect() returns the rows of final_decomposition.tsv (and, with second_best,
    of _alt.tsv) as a FinalRows instead of the raw DP rows, with identities computed on the device behind each batch.
    mono_names are required there (names are the keys: a repeated name is one key); min_identity, second_best and
    lr_coef are the command line's -i, --second-best and model coefficients (None: models/ont_logreg_model.txt, as
    the command line reads it).  formats.final_rows turns a FinalRows into FinalRow / AltRow lists.  profile=True
    (final mode only, names unique) also sums the column profiles of the kept rows: profile().

    device_rows=True (raw mode, one device): the rows of a job are assembled on the device and stay there --
    collect_device() / imap(device=True) return a DeviceRows of torch tensors; with DeviceReads input no base and no row
    passes through the host.  collect() is refused on such a stream, collect_device() on a plain one.

    device_final=True (final mode, one device): the final rows are selected on the device (csrc/sd_final_dev.hip) and
    stay there -- collect_final_device() / imap(device=True) return a DeviceFinalRows of torch tensors with the bytes
    collect() would return; with DeviceReads input no base, record or identity word passes through the host.  Jobs the
    identity words cannot decide (a block of ~19.6 kb and more, flags=FLAG_NO_STREAM_IDENT) are finished by the host's
    text-based path: the same rows, slowly (stats()["fallback_blocks"]).  Not with profile, device_rows or several devices.

    device_profile=True (with device_final, names unique): the column profiles of the kept rows are folded on the device
    from the job's text in HBM (csrc/sd_final_prof_dev.hip), behind collect_final_device(): profile() gives their sum as
    Stream(profile=True) does, profile_device() leaves it on the device.  Pairs the fold kernel does not take and jobs of
    the text-based path are folded by the host (stats()["profile_pairs_host"]).

    devices (a list of ordinals, repeats allowed; `device` is then ignored): one pipeline per entry in this process
    (sd_stream_create_devices / sd_stream_create_final_devices), each driven by a thread of its own; every job is cut
    into at least two batches per entry and the rows are those of the plain stream.  [d] is the plain stream on d."""

    def __init__(self, mono_seqs, sub_batches=1, final=False, mono_names=None, second_best=False, min_identity=0,
                 lr_coef=None, devices=None, profile=False, device_rows=False, device_final=False, device_profile=False,
                 **kw):
        self.L = load()
        if profile:
            kw["flags"] = int(kw.get("flags", 0)) | FLAG_PROFILE
        if device_rows:
            kw["flags"] = int(kw.get("flags", 0)) | FLAG_DEVICE_ROWS
        if device_final:
            kw["flags"] = int(kw.get("flags", 0)) | FLAG_DEVICE_FINAL
        if device_profile:
            kw["flags"] = int(kw.get("flags", 0)) | FLAG_DEVICE_PROFILE
        self.device_rows = bool(device_rows)
        self.device_final = bool(device_final)
        self.mono_names = None if mono_names is None else [n if isinstance(n, str) else n.decode() for n in mono_names]
        self.params = make_params(**kw)
        self._err = C.create_string_buffer(4096)
        ms = [_b(s) for s in mono_seqs]
        ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
        self.h = C.c_void_p()
        self.final = bool(final)
        self.second_best = bool(second_best)
        self.devices = None if devices is None else [int(d) for d in devices]
        devs = None if devices is None else (C.c_int32 * max(len(self.devices), 1))(*self.devices)
        if self.final:
            if mono_names is not None and len(mono_names) != len(ms):
                raise SdError(SD_ERR_PARAM, "final=True needs one name per monomer (mono_names)")
            if lr_coef is None:
                from .main import _lr_coef
                lr_coef = _lr_coef()
            coef = (C.c_double * 3)(*[float(x) for x in lr_coef])
            names = None if mono_names is None else _strs(mono_names)
            if devs is not None:
                self._check(self.L.sd_stream_create_final_devices(C.byref(self.h), C.byref(self.params), devs, len(self.devices),
                                                                  names, _strs(ms), ml, len(ms), int(sub_batches),
                                                                  int(min_identity), 1 if second_best else 0, coef, self._err, 4096))
            else:
                self._check(self.L.sd_stream_create_final(C.byref(self.h), C.byref(self.params), names, _strs(ms),
                                                          ml, len(ms), int(sub_batches), int(min_identity),
                                                          1 if second_best else 0, coef, self._err, 4096))
        elif devs is not None:
            self._check(self.L.sd_stream_create_devices(C.byref(self.h), C.byref(self.params), devs, len(self.devices),
                                                        _strs(ms), ml, len(ms), int(sub_batches), self._err, 4096))
        else:
            self._check(self.L.sd_stream_create(C.byref(self.h), C.byref(self.params), _strs(ms), ml, len(ms),
                                                int(sub_batches), self._err, 4096))
        self._n_reads = []

    def _check(self, rc):
        if rc != SD_OK:
            raise SdError(rc, self._err.value.decode(errors="replace"))

    def close(self):
        if self.h:
            self.L.sd_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, reads):
        """Enqueues a job.  The library is done with the read buffers when this returns (a final-mode stream keeps
        its own copy of the reads for the identities it computes later), so `reads` may be dropped at once."""
        if isinstance(reads, DeviceReads):   # packed on the device; the buffer is free for later work on reads.stream
            self._check(self.L.sd_stream_submit_dev(self.h, C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n,
                                                    C.c_void_p(reads.stream), self._err, 4096))
            self._n_reads.append(reads.n)
            return
        rs = reads if isinstance(reads, ReadSet) else ReadSet(reads)
        self._check(self.L.sd_stream_submit(self.h, rs.ptrs, rs.lens, rs.n, self._err, 4096))
        self._n_reads.append(rs.n)

    def profile(self, reset=False):
        """Stream(final=True, profile=True): the formats.Profile of the rows of every job processed so far (summed);
        reset=True zeroes the sums after the copy.  With device_profile=True: of every job collected so far, the device's
        counters and the host's added."""
        return _profile_from(self.L.sd_stream_profile, self.h, 1 if reset else 0)

    def profile_device(self, reset=False, stream=None):
        """Stream(device_profile=True): the sums of profile() as a DeviceProfile, placed on the stream's device by
        sd_stream_profile_dev and ordered on `stream` (a torch stream or a hipStream_t; None: the current stream of
        that device): work enqueued there afterwards sees them."""
        import torch
        nm, nc, tb = C.c_int32(), C.c_int64(), C.c_int64()
        if self.L.sd_stream_profile(self.h, 0, C.byref(nm), C.byref(nc), C.byref(tb), None, None) != SD_OK:
            raise SdError(SD_ERR_PARAM, "no profile: the stream was made without device_profile")
        text = C.create_string_buffer(max(int(tb.value), 1))
        self.L.sd_stream_profile(self.h, 0, C.byref(nm), C.byref(nc), C.byref(tb), text, None)   # (names and sequences only)
        lines = [x.split("\t") for x in text.value.decode().split("\n")[:nm.value]]
        names, seqs = [x[0] for x in lines], [x[1] for x in lines]
        offsets = [0]
        for s in seqs:
            offsets.append(offsets[-1] + (len(s) + 1) * 12)
        devs = self.devices if self.devices is not None else [self.params.device]
        dev = torch.device("cuda", devs[0])
        st = _torch_stream(torch, dev, stream)
        with torch.cuda.stream(st):
            counts = torch.empty(offsets[-1], dtype=torch.int64, device=dev)
        n = C.c_int64()
        self._check(self.L.sd_stream_profile_dev(self.h, 1 if reset else 0, C.c_void_p(counts.data_ptr()), offsets[-1],
                                                 C.c_void_p(st.cuda_stream), C.byref(n), self._err, 4096))
        return DeviceProfile(counts, offsets, names, seqs)

    def keys(self):
        """Final mode: the distinct monomer names in the library's key order (what FinalRows' indices refer to)."""
        n = C.c_int32()
        self._check(self.L.sd_stream_keys(self.h, None, 0, C.byref(n)))
        arr = (C.c_char_p * max(n.value, 1))()
        self._check(self.L.sd_stream_keys(self.h, arr, n.value, C.byref(n)))
        return [arr[i].decode() for i in range(n.value)]

    def collect(self, as_lists=False):
        """Rows of the oldest job: (n_rows,) by default -- the arrays are freed at once -- or, with
        as_lists, a list over reads of [(tmpl, start, end, score), ...].  Final mode: a FinalRows (as_lists ignored)."""
        if self.final:
            return self._collect_final()
        rows = C.POINTER(Rec)()
        off = C.POINTER(C.c_int64)()
        n = C.c_int64()
        self._check(self.L.sd_stream_collect(self.h, C.byref(rows), C.byref(off), C.byref(n), self._err, 4096))
        nr = self._n_reads.pop(0)
        out = n.value
        if as_lists:
            import numpy as np
            o = np.ctypeslib.as_array(off, shape=(nr + 1,)).copy()
            if n.value:
                r = np.frombuffer(C.string_at(rows, n.value * C.sizeof(Rec)), dtype=_rec_dtype())
            else:
                r = np.zeros(0, dtype=_rec_dtype())
            out = [[(int(x["tmpl"]), int(x["start"]), int(x["end"]), int(x["score"])) for x in r[o[i]:o[i + 1]]]
                   for i in range(nr)]
        self.L.sd_free(rows)
        self.L.sd_free(off)
        return out

    def collect_device(self, stream=None):
        """Rows of the oldest job of a device_rows stream -> DeviceRows, on the stream's device.  torch allocates the
        tensors (rows from the job's record count, an upper bound, then narrowed to n_rows) and the library fills them on
        `stream` -- a torch stream or a hipStream_t; None: the current stream of that device -- so work enqueued on it
        afterwards sees the rows and nothing waits on the host beyond the row count.  The tensors are the caller's:
        later jobs do not touch them.  torch is imported here only."""
        import torch
        devs = self.devices if self.devices is not None else [self.params.device]
        dev = torch.device("cuda", devs[0])
        st = _torch_stream(torch, dev, stream)
        nr, cap = C.c_int32(), C.c_int64()
        self._check(self.L.sd_stream_peek_dev(self.h, C.byref(nr), C.byref(cap), self._err, 4096))
        with torch.cuda.stream(st):
            rows = torch.empty((max(cap.value, 1), 4), dtype=torch.int32, device=dev)
            row_off = torch.empty(nr.value + 1, dtype=torch.int64, device=dev)
        n = C.c_int64()
        self._check(self.L.sd_stream_collect_dev(self.h, C.c_void_p(rows.data_ptr()), cap.value,
                                                 C.c_void_p(row_off.data_ptr()), C.c_void_p(st.cuda_stream), C.byref(n),
                                                 self._err, 4096))
        self._n_reads.pop(0)
        return DeviceRows(rows[:n.value], row_off, int(n.value))

    def collect_final_device(self, stream=None):
        """Final rows of the oldest job of a device_final stream -> DeviceFinalRows, on the stream's device.  The exact
        row count comes first (sd_stream_peek_final_dev), torch allocates the tensors on `stream` -- a torch stream or a
        hipStream_t; None: the current stream of that device -- and the library fills them there (collect_device's
        rules: work enqueued on the stream afterwards sees the rows, the tensors are the caller's)."""
        import torch
        devs = self.devices if self.devices is not None else [self.params.device]
        dev = torch.device("cuda", devs[0])
        st = _torch_stream(torch, dev, stream)
        nr, n, nk = C.c_int32(), C.c_int64(), C.c_int32()
        rc = self.L.sd_stream_peek_final_dev(self.h, C.byref(nr), C.byref(n), C.byref(nk), self._err, 4096)
        if rc not in (SD_OK, SD_ERR_PARAM) and self._n_reads:
            self._n_reads.pop(0)   # (a job whose rows could not be made has been dropped; a refused call leaves it)
        self._check(rc)
        with torch.cuda.stream(st):
            rows = torch.empty((n.value, 80), dtype=torch.uint8, device=dev)
            row_off = torch.empty(nr.value + 1, dtype=torch.int64, device=dev)
            alt = torch.empty((n.value, nk.value), dtype=torch.float64, device=dev) if self.second_best else None
        got = C.c_int64()
        self._check(self.L.sd_stream_collect_final_dev(self.h, C.c_void_p(rows.data_ptr() if n.value else 0), n.value,
                                                       C.c_void_p(row_off.data_ptr()),
                                                       C.c_void_p(alt.data_ptr() if alt is not None and n.value else 0),
                                                       C.c_void_p(st.cuda_stream), C.byref(got), self._err, 4096))
        self._n_reads.pop(0)
        return DeviceFinalRows(rows, row_off, alt, int(got.value))

    def collect_final_text_device(self, read_names, stream=None, tables=None):
        """collect_final_device() and format_final_device() of its rows on the same stream -> (rows, (final, alt)): a
        DeviceFinalRows and its text as DeviceText (alt None without second_best).  read_names: the job's reads in submit
        order."""
        dfr = self.collect_final_device(stream=stream)
        return dfr, format_final_device(dfr, read_names, self.keys(), stream=stream, tables=tables)

    def collect_text_device(self, read_names, stream=None, tables=None):
        """collect_device() and format_raw_device() of its rows on the same stream -> (rows, text): a DeviceRows and the
        text of its _raw.tsv as a DeviceText.  The template names come from the stream's mono_names."""
        drows = self.collect_device(stream=stream)
        return drows, format_raw_device(drows, read_names, self.tmpl_names(), stream=stream, tables=tables)

    def tmpl_names(self):
        """Column 2 of the raw TSV by template index: the monomer names, then the same names with "'"."""
        if self.mono_names is None:
            raise SdError(SD_ERR_PARAM, "the raw text needs the monomer names: Stream(..., mono_names=...)")
        return self.mono_names + [n + "'" for n in self.mono_names]

    def _collect_final(self):
        import numpy as np
        rows = C.POINTER(FinalRec)()
        off = C.POINTER(C.c_int64)()
        alt = C.POINTER(C.c_double)()
        n = C.c_int64()
        rc = self.L.sd_stream_collect_final(self.h, C.byref(rows), C.byref(off), C.byref(n), C.byref(alt), self._err, 4096)
        nr = self._n_reads.pop(0)
        try:
            self._check(rc)
            dt = final_dtype()
            r = np.frombuffer(C.string_at(rows, n.value * dt.itemsize), dtype=dt) if n.value else np.zeros(0, dtype=dt)
            o = np.ctypeslib.as_array(off, shape=(nr + 1,)).copy()
            a = None
            if self.second_best:
                nk = len(self.keys())
                a = (np.ctypeslib.as_array(alt, shape=(n.value * nk,)).copy() if n.value else np.zeros(0)).reshape(n.value, nk)
        finally:
            self.L.sd_free(rows)
            self.L.sd_free(off)
            self.L.sd_free(alt)
        return FinalRows(r, o, a)

    DEPTH = 2   # jobs outstanding before the oldest is collected: all three engines of the pipeline have a batch then

    def imap(self, jobs, as_lists=False, depth=None, device=False):
        """Rows of every job of the iterable `jobs` (read lists / ReadSets / DeviceReads), in order, with `depth` later jobs submitted
        before a job is collected -- the order of calls that keeps the device busy (sd_hip.h at sd_stream_create: the
        traceback of a batch ends with the fill of the next one, so with only ONE job outstanding the job after that is
        enqueued late; bench.py's timed loop is this generator).  device=True (a device_rows stream): every job is
        collected with collect_device() on the current stream of the stream's device and yields a DeviceRows; on a
        device_final stream with collect_final_device(), yielding a DeviceFinalRows.

        The default depth is DEPTH = 2 with a device list too.  There every job is cut into at least two batches per
        entry, so two jobs outstanding give each entry at least four batches -- more than its pipeline's three slots --
        and while the oldest job is collected the other still holds two batches per entry, back to back, which is what
        one pipeline gets from two single-batch jobs.  A deeper queue would only hold more reads and rows in memory
        (a raw-mode submit already waits until its batches are packed, so it cannot run far ahead of the devices)."""
        depth = self.DEPTH if depth is None else max(0, int(depth))
        collect = lambda: self.collect(as_lists=as_lists)   # noqa: E731
        if device:   # DeviceRows / DeviceFinalRows
            collect = self.collect_final_device if self.device_final else self.collect_device
        out = 0
        for reads in jobs:
            self.submit(reads)
            out += 1
            if out > depth:
                out -= 1
                yield collect()
        while out > 0:
            out -= 1
            yield collect()

    def stats(self):
        v = (C.c_double * 16)()
        self.L.sd_stream_stats(self.h, v)
        keys = ["fill_ms", "trace_ms", "compact_ms", "run_ms", "fill_launches", "batches", "rows", "host_pack_ms",
                "host_wait_ms", "host_assemble_ms", "submit_ms", "collect_ms", "jobs", "sub_batches", "row_budget"]
        out = dict(zip(keys, list(v)[:15]))
        f = (C.c_double * 4)()
        self.L.sd_stream_final_stats(self.h, f)
        out.update({"ident_ms": f[0], "ident_pairs": int(f[1]), "fallback_blocks": int(f[2]), "final_rows": int(f[3])})
        self.L.sd_stream_profile_stats(self.h, f)
        out.update({"profile_pairs_device": int(f[0]), "profile_pairs_host": int(f[1]), "profile_text_to_host": int(f[2]),
                    "profile_ms": f[3]})
        return out

    def info(self):
        v = (C.c_int64 * 8)()
        self.L.sd_stream_info(self.h, v)
        return _info_dict(v)

    def device_stats(self):
        """Per entry of the stream (one without a device list; sd_stream_device_stats): a list of {"device",
        "batches": batches dealt to the entry, "busy_ms": its device busy time (HIP-event spans of its batches)}."""
        b = (C.c_int64 * 16)()
        ms = (C.c_double * 16)()
        n = self.L.sd_stream_device_stats(self.h, b, ms, 16)
        devs = self.devices if self.devices is not None else [self.params.device]
        return [{"device": devs[i], "batches": int(b[i]), "busy_ms": float(ms[i])} for i in range(min(n, 16))]


def host_stage_rates(reads, iters=3, **kw):
    """{"pack_bp_per_s", "assemble_format_bp_per_s", "rows_per_s", "text_bytes"} of the host stages alone."""
    L = load()
    rs = reads if isinstance(reads, ReadSet) else ReadSet(reads)
    p = make_params(**kw)
    out = (C.c_double * 4)()
    rc = L.sd_host_stage_rates(rs.ptrs, rs.lens, rs.n, C.byref(p), int(iters), out)
    if rc != SD_OK:
        raise SdError(rc, "sd_host_stage_rates")
    return {"pack_bp_per_s": out[0], "assemble_format_bp_per_s": out[1], "rows_per_s": out[2], "text_bytes": out[3]}


def write_parts_selftest(path, n_parts, part_bytes, threads=4, fail_reserve=False):
    """sd::write_parts alone (the file writer of sd_run_files); returns (bytes written, on tmpfs)."""
    L = load()
    L.sd_write_parts_selftest.restype = C.c_int
    L.sd_write_parts_selftest.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 2)()
    rc = L.sd_write_parts_selftest(_b(path), n_parts, part_bytes, threads, 1 if fail_reserve else 0, out)
    if rc != SD_OK:
        raise SdError(rc, "sd_write_parts_selftest")
    return int(out[0]), bool(out[1])


def pack_bases(seq):
    """(words uint32[(n+15)//16], nmask uint32[(n+31)//32], has_n) exactly as the device reads a chunk."""
    import numpy as np
    L = load()
    b = _b(seq)
    w = np.zeros((len(b) + 15) // 16, dtype=np.uint32)
    m = np.zeros((len(b) + 31) // 32, dtype=np.uint32)
    rc = L.sd_pack_bases(b, len(b), w.ctypes.data, m.ctypes.data)
    if rc < 0:
        raise SdError(SD_ERR_PARAM, "sd_pack_bases")
    return w, m, bool(rc)


def format_rows(read_name, tmpl_names, rows):
    L = load()
    arr = (Rec * max(len(rows), 1))()
    for i, r in enumerate(rows):
        arr[i] = Rec(*[int(x) for x in r])
    out = C.c_void_p()
    ln = C.c_size_t()
    rc = L.sd_format_rows(_b(read_name), _strs(tmpl_names), arr, len(rows), C.byref(out), C.byref(ln))
    if rc != SD_OK:
        raise SdError(rc, "sd_format_rows")
    data = C.string_at(out, ln.value)
    L.sd_free(out)
    return data


def chunk_plan(length, part=5000, overlap=500):
    L = load()
    n = L.sd_chunk_plan(length, part, overlap, None, None, 0)
    off = (C.c_int64 * max(n, 1))()
    ln = (C.c_int32 * max(n, 1))()
    L.sd_chunk_plan(length, part, overlap, off, ln, n)
    return [(off[i], ln[i]) for i in range(n)]


def seam_merge(recs):
    L = load()
    arr = (Rec * max(len(recs), 1))()
    for i, r in enumerate(recs):
        arr[i] = Rec(*[int(x) for x in r])
    m = L.sd_seam_merge(arr, len(recs))
    return [(arr[i].tmpl, arr[i].start, arr[i].end, arr[i].score) for i in range(m)]


def _recs_array(recs, read_off):
    import numpy as np
    r = np.ascontiguousarray(recs, dtype=np.int32).reshape(-1, 4)
    o = np.ascontiguousarray(read_off, dtype=np.int64)
    if o.ndim != 1 or len(o) < 1 or int(o[-1]) != len(r):
        raise SdError(SD_ERR_PARAM, "read_off: n_reads + 1 offsets, the last = the number of records")
    return r, o


def seam_pieces_host(recs, read_off, piece=0):
    """The piecewise seam merge run by the host (sd_seam_pieces_selftest: the functions the device kernels run).
    recs: [n, 4] int32 (tmpl, start, end, score), read-global; read_off: n_reads + 1 offsets from 0; piece: records
    per piece, 0 = the production value.  -> (rows [m, 4], row_off)."""
    import numpy as np
    r, o = _recs_array(recs, read_off)
    rows = np.empty((max(len(r), 1), 4), dtype=np.int32)
    row_off = np.empty(len(o), dtype=np.int64)
    n = C.c_int64()
    rc = load().sd_seam_pieces_selftest(r.ctypes.data, o.ctypes.data, len(o) - 1, int(piece), rows.ctypes.data,
                                        row_off.ctypes.data, C.byref(n))
    if rc != SD_OK:
        raise SdError(rc, "sd_seam_pieces_selftest")
    return rows[:n.value], row_off


def scan_selftest(values, tile_sums_32=False, device=0):
    """The device prefix scan of the post-pass units alone (sd_scan_selftest): values: n int64 counts ->
    n + 1 int64, out[i] = the sum of values[:i].  tile_sums_32: keep the sums per tile as int32."""
    import numpy as np
    v = np.ascontiguousarray(values, dtype=np.int64)
    out = np.empty(len(v) + 1, dtype=np.int64)
    L = load()
    L.sd_scan_selftest.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    rc = L.sd_scan_selftest(v.ctypes.data, len(v), 1 if tile_sums_32 else 0, int(device), out.ctypes.data)
    if rc != SD_OK:
        raise SdError(rc, "sd_scan_selftest")
    return out


def seam_merge_device(recs, read_off, piece=0, device=0, stream=None, pad=0):
    """The assembly kernels alone (sd_seam_merge_dev), arguments as seam_pieces_host; the arrays go to `device` through
    torch and the results come back as numpy.  pad: sentinel words put before and after both outputs on the device;
    with pad > 0 the result is (rows, row_off, intact) where intact tells whether every sentinel survived."""
    import numpy as np
    import torch
    r, o = _recs_array(recs, read_off)
    dev = torch.device("cuda", int(device))
    st = _torch_stream(torch, dev, stream)
    pad = int(pad)
    with torch.cuda.stream(st):
        d_r = torch.from_numpy(r).to(dev)
        d_o = torch.from_numpy(o).to(dev)
        d_rows = torch.full((len(r) + 2 * pad, 4), -559038737, dtype=torch.int32, device=dev)
        d_off = torch.full((len(o) + 2 * pad,), -559038737, dtype=torch.int64, device=dev)
        n = C.c_int64()
        rc = load().sd_seam_merge_dev(C.c_void_p(d_r.data_ptr()), C.c_void_p(d_o.data_ptr()), len(o) - 1, int(piece),
                                      int(device), C.c_void_p(st.cuda_stream), C.c_void_p(d_rows.data_ptr() + 16 * pad),
                                      C.c_void_p(d_off.data_ptr() + 8 * pad), C.byref(n))
        if rc != SD_OK:
            raise SdError(rc, "sd_seam_merge_dev")
        h_rows, h_off = d_rows.cpu().numpy(), d_off.cpu().numpy()
    rows, row_off = h_rows[pad:pad + n.value], h_off[pad:pad + len(o)]
    if not pad:
        return rows, row_off
    intact = bool((h_rows[:pad] == -559038737).all() and (h_rows[pad + n.value:] == -559038737).all()
                  and (h_off[:pad] == -559038737).all() and (h_off[pad + len(o):] == -559038737).all())
    return rows, row_off, intact


def _final_select_args(mono_names, mono_seqs, min_identity, second_best, lr_coef):
    ms = [_b(s) for s in mono_seqs]
    if lr_coef is None:
        from .main import _lr_coef
        lr_coef = _lr_coef()
    return [_strs(mono_names), _strs(ms), (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms]), len(ms), int(min_identity),
            1 if second_best else 0, (C.c_double * 3)(*[float(x) for x in lr_coef])]


def _final_select_arrays(rows, row_off, widx, words, hwords, read_len, second_best, n_mono):
    import numpy as np
    r, o = _recs_array(rows, row_off)
    per = 2 * n_mono if second_best else 1
    wi = np.ascontiguousarray(widx, dtype=np.int64)
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, per)
    h = np.ascontiguousarray(hwords, dtype=np.uint32).reshape(-1, per) if second_best else None
    if len(wi) != len(r) or (h is not None and h.shape != w.shape):
        raise SdError(SD_ERR_PARAM, "final_select: one word index per row, hwords shaped as words")
    rl = None if read_len is None else np.ascontiguousarray(read_len, dtype=np.int64)
    if rl is not None and len(rl) != len(o) - 1:
        raise SdError(SD_ERR_PARAM, "final_select: one length per read")
    return r, o, wi, w, h, rl, per


def final_select_host(mono_names, mono_seqs, rows, row_off, widx, words, hwords=None, read_len=None, min_identity=0,
                      second_best=False, lr_coef=None):
    """The host's selection alone on identity words (sd_final_select_host).  rows: [n, 4] int32 (tmpl, start, end,
    score), merged, read-global; row_off: n_reads + 1 offsets; widx: per row, which row of words / hwords holds its words
    ([n_word_rows, per] uint32, per = 1 or, with second_best, 2 * monomers).  -> (FinalRows, n_undecided)."""
    import numpy as np
    r, o, wi, w, h, rl, per = _final_select_arrays(rows, row_off, widx, words, hwords, read_len, second_best, len(mono_seqs))
    nk = len(dict.fromkeys(x for n in mono_names for x in (n, n + "'")))
    out = np.zeros(max(len(r), 1), dtype=final_dtype())
    out_off = np.zeros(len(o), dtype=np.int64)
    alt = np.zeros((max(len(r), 1), nk), dtype=np.float64) if second_best else None
    n, und = C.c_int64(), C.c_int64()
    rc = load().sd_final_select_host(*_final_select_args(mono_names, mono_seqs, min_identity, second_best, lr_coef),
                                     r.ctypes.data, o.ctypes.data, len(o) - 1, wi.ctypes.data, w.ctypes.data,
                                     h.ctypes.data if h is not None else None, len(w), per,
                                     rl.ctypes.data if rl is not None else None, out.ctypes.data, out_off.ctypes.data,
                                     alt.ctypes.data if alt is not None else None, C.byref(n), C.byref(und))
    if rc != SD_OK:
        raise SdError(rc, "sd_final_select_host")
    return FinalRows(out[:n.value], out_off, None if alt is None else alt[:n.value]), int(und.value)


def final_select_device(mono_names, mono_seqs, rows, row_off, widx, words, hwords=None, read_len=None, min_identity=0,
                        second_best=False, lr_coef=None, device=0, stream=None):
    """The selection kernels alone (sd_final_select_dev), arguments and result as final_select_host; the arrays go to
    `device` through torch and the results come back as numpy.  Every output buffer carries guard bytes behind it: the
    result is (FinalRows, n_undecided, intact)."""
    import numpy as np
    r, o, wi, w, h, rl, per = _final_select_arrays(rows, row_off, widx, words, hwords, read_len, second_best, len(mono_seqs))
    nk = len(dict.fromkeys(x for n in mono_names for x in (n, n + "'")))
    torch, dev, st = _device_frame(int(device), stream)
    G = 0x5a
    with torch.cuda.stream(st):
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)   # noqa: E731
        d_r, d_o, d_wi, d_w, d_h, d_rl = up(r), up(o), up(wi), up(w), up(h), up(rl)
        d_out = torch.full(((len(r) + 1) * 80,), G, dtype=torch.uint8, device=dev)
        d_off = torch.full(((len(o) + 1) * 8,), G, dtype=torch.uint8, device=dev)
        d_alt = torch.full(((len(r) * nk + 1) * 8,), G, dtype=torch.uint8, device=dev) if second_best else None
        n, und = C.c_int64(), C.c_int64()
        rc = load().sd_final_select_dev(*_final_select_args(mono_names, mono_seqs, min_identity, second_best, lr_coef),
                                        _dptr(d_r), _dptr(d_o), len(o) - 1, _dptr(d_wi), _dptr(d_w), _dptr(d_h), len(w), per,
                                        _dptr(d_rl), int(device), C.c_void_p(st.cuda_stream), _dptr(d_out), _dptr(d_off),
                                        _dptr(d_alt), C.byref(n), C.byref(und))
        _check(rc, "sd_final_select_dev")
        h_out, h_off = d_out.cpu().numpy(), d_off.cpu().numpy()
        h_alt = d_alt.cpu().numpy() if d_alt is not None else None
    k = n.value
    intact = bool((h_out[k * 80:] == G).all() and (h_off[len(o) * 8:] == G).all()
                  and (h_alt is None or (h_alt[k * nk * 8:] == G).all()))
    out = h_out[:k * 80].copy().view(final_dtype())
    alt = None if h_alt is None else h_alt[:k * nk * 8].copy().view(np.float64).reshape(k, nk)
    return FinalRows(out, h_off[:len(o) * 8].copy().view(np.int64), alt), int(und.value), intact


def _final_profile(fn, name, text, read_off, rows, row_off, keep, templates, device, threads, guard):
    import numpy as np
    from . import formats
    tb = _b(text)
    ro = np.ascontiguousarray(read_off, dtype=np.int64)
    r, o = _recs_array(rows, row_off)
    k = np.ascontiguousarray(keep, dtype=np.uint8)
    if len(ro) != len(o) or len(k) != len(r) or (len(ro) and int(ro[-1]) > len(tb)):
        raise SdError(SD_ERR_PARAM, name + ": one keep flag per row, n_reads + 1 offsets of reads and of rows, inside the text")
    ts = [_b(t) for t in templates]
    tl = (C.c_int32 * max(len(ts), 1))(*[len(t) for t in ts])
    total = sum(len(t) + 1 for t in ts) * formats.PROFILE_NCOLS
    counts = np.full(total + guard, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    pairs = (C.c_int64 * 2)()
    rc = fn(tb, ro.ctypes.data, len(ro) - 1, r.ctypes.data, o.ctypes.data, k.ctypes.data, _strs(ts), tl, len(ts), int(device),
            int(threads), counts.ctypes.data, pairs)
    if rc != SD_OK:
        raise SdError(rc, name)
    intact = bool((counts[total:] == 0x5a5a5a5a5a5a5a5a).all())
    return formats.split_counts([len(t) for t in ts], counts[:total].astype(np.int64)), (int(pairs[0]), int(pairs[1])), intact


def final_profile_host(text, read_off, rows, row_off, keep, templates, threads=1):
    """The plan of a device-final stream's profiles on the host (sd_final_profile_host): text = the reads back to back,
    read r = text[read_off[r]:read_off[r + 1]]; rows [n, 4] int32 (tmpl in the DP's order: monomer t, T + t = its
    reverse complement; start, end in read coordinates), row_off n_reads + 1 offsets, keep one flag per row; templates =
    the FORWARD monomers.  -> (counts as profile_segments gives them, (pairs of the fold kernel, pairs of the host))."""
    c, pairs, _ = _final_profile(load().sd_final_profile_host, "sd_final_profile_host", text, read_off, rows, row_off, keep,
                                 templates, 0, threads, 0)
    return c, pairs


def final_profile_device(text, read_off, rows, row_off, keep, templates, device=0, threads=1):
    """The plan, group and fold kernels alone (sd_final_profile_dev), arguments as final_profile_host.  The count buffer
    carries guard words behind it: -> (counts, pairs, intact)."""
    return _final_profile(load().sd_final_profile_dev, "sd_final_profile_dev", text, read_off, rows, row_off, keep, templates,
                          device, threads, 16)


def fasta_load(path, lenient=False):
    """-> (names, seqs, has_n) with the reference binary's FASTA semantics (main.cpp:314-346).  A file that begins with
    '@' is read as four-line FASTQ.  lenient=True (sd_fasta_load_ex with SD_FLAG_LENIENT): lower case is folded, IUPAC
    ambiguity codes become N and the CR of a CRLF line end is dropped; has_n reflects the normalised text."""
    L = load()
    f = Fasta()
    err = C.create_string_buffer(4096)
    rc = L.sd_fasta_load_ex(os.fsencode(path), FLAG_LENIENT if lenient else 0, C.byref(f), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    names = [f.names[i].decode() for i in range(f.n)]
    seqs = [C.string_at(f.seqs[i], f.lens[i]) for i in range(f.n)]
    has_n = bool(f.has_n)
    L.sd_fasta_free(C.byref(f))
    return names, seqs, has_n


def nw_identity_batch(queries, targets, threads=1):
    """[(dist, matches, columns)] of unit-cost NW alignments (main.py:29-60 semantics)."""
    L = load()
    n = len(queries)
    q = [_b(s) for s in queries]
    t = [_b(s) for s in targets]
    ql = (C.c_int32 * max(n, 1))(*[len(s) for s in q])
    tl = (C.c_int32 * max(n, 1))(*[len(s) for s in t])
    d = (C.c_int32 * max(n, 1))()
    m = (C.c_int32 * max(n, 1))()
    c = (C.c_int32 * max(n, 1))()
    rc = L.sd_nw_identity_batch(_strs(q), ql, _strs(t), tl, n, threads, d, m, c)
    if rc != SD_OK:
        raise SdError(rc, "sd_nw_identity_batch")
    return [(d[i], m[i], c[i]) for i in range(n)]


def identity_segments(seq, starts, ends, templates, homo=False, threads=1, pair_tmpl=None, device=None):
    """(dist, matches, columns) int32 arrays of shape [n_segments, n_templates]: every segment
    seq[starts[s] .. ends[s]] (inclusive) against every template (main.py:107-150 all-vs-all);
    with pair_tmpl (template index per segment) arrays of shape [n_segments]: that pair only.
    device=None: the host implementation (sd_identity_segments); device=<ordinal>: the HIP kernel
    (sd_identity_segments_dev), with the host implementation for input the kernel does not take."""
    import numpy as np
    L = load()
    seg = _segments(None, seq, starts, ends, pair_tmpl=pair_tmpl, templates=templates)
    shape = (seg.n, len(seg.tb)) if seg.pt is None else (seg.n,)
    d = np.zeros(shape, dtype=np.int32)
    m = np.zeros(shape, dtype=np.int32)
    c = np.zeros(shape, dtype=np.int32)
    rc = SD_ERR_UNSUPPORTED
    if device is not None:
        rc = L.sd_identity_segments_dev(*seg.lead, 1 if homo else 0, int(device), threads, d.ctypes.data, m.ctypes.data, c.ctypes.data)
        if rc != SD_ERR_UNSUPPORTED:
            _check(rc, "sd_identity_segments_dev")
    if rc == SD_ERR_UNSUPPORTED:
        rc = L.sd_identity_segments(*seg.lead, 1 if homo else 0, threads, d.ctypes.data, m.ctypes.data, c.ctypes.data)
    _check(rc, "sd_identity_segments")
    return d, m, c


# ---- chunk-range form (one job over several GPUs, one process per GPU; see shard.py) ---------------
def _rec_dtype():
    import numpy as np
    return np.dtype([("tmpl", np.int32), ("start", np.int32), ("end", np.int32), ("score", np.int32)])


def chunk_table_size(read_lens, part_size=5000, overlap=500):
    L = load()
    arr = (C.c_int64 * max(len(read_lens), 1))(*[int(x) for x in read_lens])
    return L.sd_chunk_table_size(arr, len(read_lens), part_size, overlap)


def decompose_chunk_range(read_seqs, mono_seqs, chunk_lo, chunk_hi, **kw):
    """Records of the chunks [chunk_lo, chunk_hi) of the global chunk table of `read_seqs`:
    (recs structured array [tmpl, start, end, score], rec_off int64[chunk_hi - chunk_lo + 1])."""
    import numpy as np
    L = load()
    p = make_params(**kw)
    rs = [_b(s) for s in read_seqs]
    ms = [_b(s) for s in mono_seqs]
    rl = (C.c_int64 * max(len(rs), 1))(*[len(s) for s in rs])
    ml = (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])
    recs = C.POINTER(Rec)()
    off = C.POINTER(C.c_int64)()
    err = C.create_string_buffer(4096)
    rc = L.sd_decompose_chunk_range(_strs(rs), rl, len(rs), _strs(ms), ml, len(ms), C.byref(p), chunk_lo,
                                    chunk_hi, C.byref(recs), C.byref(off), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    n = chunk_hi - chunk_lo
    o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
    nrec = int(o[n])
    if nrec:   # one copy out of the library's buffer
        r = np.ctypeslib.as_array(C.cast(recs, C.POINTER(C.c_int32)), shape=(nrec * 4,)).copy().view(_rec_dtype())
    else:
        r = np.zeros(0, dtype=_rec_dtype())
    L.sd_free(recs)
    L.sd_free(off)
    return r, o


def decompose_files_range(reads_fa, monomers_fa, rank, world, **kw):
    """A rank's share of a sharded job straight from the FASTA files (mapped, not copied):
    (recs, rec_off, chunk_lo, chunk_hi, n_chunks_total)."""
    import numpy as np
    L = load()
    p = make_params(**kw)
    recs = C.POINTER(Rec)()
    off = C.POINTER(C.c_int64)()
    lo, hi, tot = C.c_int64(), C.c_int64(), C.c_int64()
    err = C.create_string_buffer(4096)
    rc = L.sd_decompose_files_range(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), rank, world,
                                    C.byref(recs), C.byref(off), C.byref(lo), C.byref(hi), C.byref(tot), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    n = hi.value - lo.value
    o = np.ctypeslib.as_array(off, shape=(n + 1,)).copy()
    nrec = int(o[n])
    r = (np.frombuffer(C.string_at(recs, nrec * C.sizeof(Rec)), dtype=_rec_dtype()).copy() if nrec
         else np.zeros(0, dtype=_rec_dtype()))
    L.sd_free(recs)
    L.sd_free(off)
    return r, o, lo.value, hi.value, tot.value


def assemble_files_tsv(reads_fa, monomers_fa, recs, rec_off, raw_tsv_out, **kw):
    """Rank 0: gathered records of all chunks -> raw TSV file (names / lengths from the FASTA index)."""
    import numpy as np
    L = load()
    p = make_params(**kw)
    r = np.ascontiguousarray(recs, dtype=_rec_dtype())
    o = np.ascontiguousarray(rec_off, dtype=np.int64)
    err = C.create_string_buffer(4096)
    rc = L.sd_assemble_files_tsv(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), r.ctypes.data,
                                 o.ctypes.data, len(o) - 1, os.fsencode(raw_tsv_out), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))


class SeamEdge(C.Structure):
    """sd_seam_edge (include/sd_hip.h): what a rank publishes about the records either side of its range boundaries."""
    _fields_ = [("ok", C.c_int32), ("has_front", C.c_int32), ("has_back", C.c_int32), ("through", C.c_int32),
                ("head", (C.c_int32 * 2) * 8), ("tail", (C.c_int32 * 2) * 8), ("exit_of", C.c_int8 * 8),
                ("reserved", C.c_int64)]


class RangeAssembler:
    """One rank's part of the raw TSV of a job sharded by chunk range (sd_range_assemble_*, include/sd_hip.h):
         a = RangeAssembler.from_files(reads_fa, monomers_fa, rank, world, recs, rec_off, **params)   # or .from_lists
         edges = <all-gather of a.edge (bytes)>
         nbytes = a.text(edges)            # SdError(SD_ERR_UNSUPPORTED): gather on rank 0 instead
         a.write(path, offset) / a.bytes()
    Host only; the concatenation of the ranks' texts equals assemble_tsv of all records."""

    def __init__(self, handle, edge, keep):
        self._h = handle
        self._keep = keep
        self.edge = bytes(edge)
        self.nbytes = None

    @staticmethod
    def _bind(L):
        L.sd_range_assemble_begin.restype = C.c_int
        L.sd_range_assemble_begin_files.restype = C.c_int
        L.sd_range_assemble_text.restype = C.c_int
        L.sd_range_assemble_write.restype = C.c_int
        L.sd_range_assemble_copy.restype = C.c_int
        L.sd_range_assemble_stats.restype = None
        L.sd_range_assemble_free.restype = None
        L.sd_range_assemble_free.argtypes = [C.c_void_p]
        L.sd_range_assemble_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.sd_range_assemble_text.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_size_t]
        L.sd_range_assemble_write.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]
        L.sd_decompose_files_range_begin.restype = C.c_int
        L.sd_range_assemble_records.restype = C.c_int
        L.sd_range_assemble_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]

    @classmethod
    def from_files(cls, reads_fa, monomers_fa, rank, world, recs, rec_off, **kw):
        import numpy as np
        L = load()
        cls._bind(L)
        p = make_params(**kw)
        r = np.ascontiguousarray(recs, dtype=_rec_dtype())
        o = np.ascontiguousarray(rec_off, dtype=np.int64)
        edge, h = SeamEdge(), C.c_void_p()
        err = C.create_string_buffer(4096)
        rc = L.sd_range_assemble_begin_files(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), C.c_int32(rank),
                                             C.c_int32(world), C.c_void_p(r.ctypes.data), C.c_void_p(o.ctypes.data),
                                             C.byref(edge), C.byref(h), err, C.c_size_t(4096))
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        return cls(h, edge, (r, o))

    @classmethod
    def run_files(cls, reads_fa, monomers_fa, rank, world, **kw):
        """DP of this rank's share + step 1 in one library call (sd_decompose_files_range_begin): the records stay in the
        library.  Sets .chunk_lo / .chunk_hi / .n_chunks; .records() copies the records out for the gather fall-back."""
        L = load()
        cls._bind(L)
        p = make_params(**kw)
        edge, h = SeamEdge(), C.c_void_p()
        lo, hi, tot = C.c_int64(), C.c_int64(), C.c_int64()
        err = C.create_string_buffer(4096)
        rc = L.sd_decompose_files_range_begin(os.fsencode(reads_fa), os.fsencode(monomers_fa), C.byref(p), C.c_int32(rank),
                                              C.c_int32(world), C.byref(edge), C.byref(h), C.byref(lo), C.byref(hi),
                                              C.byref(tot), err, C.c_size_t(4096))
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        a = cls(h, edge, None)
        a.chunk_lo, a.chunk_hi, a.n_chunks = lo.value, hi.value, tot.value
        return a

    def records(self):
        """(recs, rec_off) of the share held by the library (copies)."""
        import numpy as np
        L = load()
        recs, off, n = C.POINTER(Rec)(), C.POINTER(C.c_int64)(), C.c_int64()
        rc = L.sd_range_assemble_records(self._h, C.byref(recs), C.byref(off), C.byref(n))
        if rc != SD_OK:
            raise SdError(rc, "this assembler does not hold its records")
        o = np.ctypeslib.as_array(off, shape=(n.value + 1,)).copy()
        nrec = int(o[n.value])
        r = (np.frombuffer(C.string_at(recs, nrec * C.sizeof(Rec)), dtype=_rec_dtype()).copy() if nrec
             else np.zeros(0, dtype=_rec_dtype()))
        return r, o

    @classmethod
    def from_lists(cls, read_names, read_lens, mono_names, chunk_lo, chunk_hi, recs, rec_off, **kw):
        import numpy as np
        L = load()
        cls._bind(L)
        p = make_params(**kw)
        rn = [_b(s) for s in read_names]
        mn = [_b(s) for s in mono_names]
        rl = (C.c_int64 * max(len(rn), 1))(*[int(x) for x in read_lens])
        r = np.ascontiguousarray(recs, dtype=_rec_dtype())
        o = np.ascontiguousarray(rec_off, dtype=np.int64)
        edge, h = SeamEdge(), C.c_void_p()
        err = C.create_string_buffer(4096)
        rc = L.sd_range_assemble_begin(_strs(rn), rl, C.c_int32(len(rn)), _strs(mn), C.c_int32(len(mn)), C.byref(p),
                                       C.c_int64(chunk_lo), C.c_int64(chunk_hi), C.c_void_p(r.ctypes.data),
                                       C.c_void_p(o.ctypes.data), C.byref(edge), C.byref(h), err, C.c_size_t(4096))
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        return cls(h, edge, (r, o))

    def text(self, edges, rank):
        """edges: the edges of all ranks in rank order (bytes each).  Returns the bytes of this rank's text."""
        L = load()
        arr = (SeamEdge * len(edges))()
        for k, e in enumerate(edges):
            if e is None or len(e) != C.sizeof(SeamEdge):
                raise SdError(SD_ERR_UNSUPPORTED, "a rank published no edge")
            C.memmove(C.byref(arr[k]), e, C.sizeof(SeamEdge))
        n = C.c_int64()
        err = C.create_string_buffer(4096)
        rc = L.sd_range_assemble_text(self._h, arr, len(edges), int(rank), C.byref(n), err, 4096)
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))
        self.nbytes = n.value
        return n.value

    def write(self, path, offset, file_bytes=-1):
        """file_bytes >= 0: create the file if missing and set its size first (every rank passes the same total)."""
        L = load()
        err = C.create_string_buffer(4096)
        rc = L.sd_range_assemble_write(self._h, os.fsencode(path), int(offset), int(file_bytes), err, 4096)
        if rc != SD_OK:
            raise SdError(rc, err.value.decode(errors="replace"))

    def bytes(self):
        L = load()
        buf = C.create_string_buffer(max(self.nbytes, 1))
        rc = L.sd_range_assemble_copy(self._h, buf, self.nbytes)
        if rc != SD_OK:
            raise SdError(rc, "sd_range_assemble_copy")
        return buf.raw[:self.nbytes]

    def stats(self):
        L = load()
        out = (C.c_double * 8)()
        L.sd_range_assemble_stats(self._h, out)
        return {"begin_ms": out[0], "complete_reads_ms": out[1], "assumed_scan_and_text_ahead_ms": out[2],
                "text_ms": out[3], "rows_printed_after_exchange": int(out[4]), "formatted_again": bool(out[5]),
                "write_ms": out[6]}

    def close(self):
        if self._h:
            load().sd_range_assemble_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assemble_tsv(read_names, read_lens, mono_names, recs, rec_off, **kw):
    """Raw TSV bytes from the records of all chunks in table order (host only)."""
    import numpy as np
    L = load()
    p = make_params(**kw)
    rn = [_b(s) for s in read_names]
    mn = [_b(s) for s in mono_names]
    rl = (C.c_int64 * max(len(rn), 1))(*[int(x) for x in read_lens])
    r = np.ascontiguousarray(recs, dtype=_rec_dtype())
    o = np.ascontiguousarray(rec_off, dtype=np.int64)
    out = C.c_void_p()
    ln = C.c_size_t()
    err = C.create_string_buffer(4096)
    rc = L.sd_assemble_tsv(_strs(rn), rl, len(rn), _strs(mn), len(mn), C.byref(p), r.ctypes.data,
                           o.ctypes.data, len(o) - 1, C.byref(out), C.byref(ln), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    data = C.string_at(out, ln.value)
    L.sd_free(out)
    return data


def format_alt_rows(read_name, key_names, starts, ends, own_key, vals, threads=1, row_read=None):
    """Text (str) of _alt.tsv rows; vals is a [n_rows, n_keys] float64 array.  read_name: one name, or a
    list of names with row_read giving each row's index into it."""
    import numpy as np
    L = load()
    names = [read_name] if isinstance(read_name, (str, bytes)) else list(read_name)
    rr = None if row_read is None else np.ascontiguousarray(row_read, dtype=np.int32)
    v = np.ascontiguousarray(vals, dtype=np.float64)
    n, nk = (int(v.shape[0]), int(v.shape[1])) if v.ndim == 2 else (0, len(key_names))
    st = np.ascontiguousarray(starts, dtype=np.int64)
    en = np.ascontiguousarray(ends, dtype=np.int64)
    ow = np.ascontiguousarray(own_key, dtype=np.int32)
    out = C.c_void_p()
    ln = C.c_size_t()
    rc = L.sd_format_alt_rows(_strs([_b(x) for x in names]), len(names), None if rr is None else rr.ctypes.data,
                              _strs([_b(k) for k in key_names]), nk, st.ctypes.data, en.ctypes.data,
                              ow.ctypes.data, v.ctypes.data, n, threads, C.byref(out), C.byref(ln))
    if rc != SD_OK:
        raise SdError(rc, "sd_format_alt_rows")
    data = C.string_at(out, ln.value).decode()
    L.sd_free(out)
    return data


# ---- the screen: decompose only the stretches where a monomer occurs (csrc/sd_screen.hip) ----------------------------
ScreenKeys = namedtuple("ScreenKeys", "chunk_read chunk_off chunk_len key")
"""The chunks of a read set in chunk-table order: chunk_read (int32), chunk_off (int64, in the read), chunk_len (int32)
and key (uint32: (smallest infix edit distance of a template against the chunk) << 16 | the first template that has
it; templates = the monomers, then their reverse complements).  key is a numpy array, or an int32 torch tensor on the
device (the same bits) when Screener.chunks(device_out=True) made it."""


def screen_region_dtype():
    """numpy dtype of sd_screen_region (include/sd_hip.h)."""
    import numpy as np
    return np.dtype([("read", "<i4"), ("start", "<i8"), ("end_incl", "<i8"), ("n_chunks", "<i4"), ("best_key", "<u4")],
                    align=True)


def chunk_table(read_lens, part_size=5000, overlap=500):
    """(chunk_read, chunk_off, chunk_len) of the reads' standard chunk plan (main.cpp:70-81), as numpy arrays."""
    import numpy as np
    cr, co, cl = [], [], []
    for r, n in enumerate(read_lens):
        for o, ln in chunk_plan(int(n), int(part_size), int(overlap)):
            cr.append(r)
            co.append(o)
            cl.append(ln)
    return np.array(cr, dtype=np.int32), np.array(co, dtype=np.int64), np.array(cl, dtype=np.int32)


def _mono_args(mono_seqs):
    ms = [_b(s) for s in mono_seqs]
    return ms, _strs(ms), (C.c_int32 * max(len(ms), 1))(*[len(s) for s in ms])


def screen_chunks_host(mono_seqs, reads, part_size=5000, overlap=500):
    """The screen's keys without a device (sd_screen_chunks_host: a plain DP, exact and slow) -> ScreenKeys."""
    import numpy as np
    L = load()
    ms, mp, ml = _mono_args(mono_seqs)
    rs = reads if isinstance(reads, ReadSet) else ReadSet(reads)
    cr, co, cl = chunk_table([len(s) for s in rs.seqs], part_size, overlap)
    key = np.zeros(max(len(cr), 1), dtype=np.uint32)
    n = C.c_int64()
    err = C.create_string_buffer(4096)
    rc = L.sd_screen_chunks_host(mp, ml, len(ms), rs.ptrs, rs.lens, rs.n, int(part_size), int(overlap), key.ctypes.data,
                                 len(key), C.byref(n), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    assert n.value == len(cr)
    return ScreenKeys(cr, co, cl, key[:len(cr)])


class Screener:
    """The screen on one device (sd_screen_*): the handle holds the templates, their match masks and scratch.
    chunks() gives one key per chunk of the reads' chunk plan; screen_regions() turns keys and a threshold into regions,
    region_reads() / rows_from_regions() carry them through an unchanged Stream or Engine."""

    def __init__(self, mono_seqs, device=0, general=False):
        self.L = load()
        self._err = C.create_string_buffer(4096)
        ms, mp, ml = _mono_args(mono_seqs)
        self.h = C.c_void_p()
        self.device = int(device)
        self._check(self.L.sd_screen_create(mp, ml, len(ms), self.device, C.byref(self.h), self._err, 4096))
        if general:   # the general distance kernel where the uniform one would run (A/B, tests)
            self._check(self.L.sd_screen_set_general(self.h, 1))

    def _check(self, rc):
        if rc != SD_OK:
            raise SdError(rc, self._err.value.decode(errors="replace"))

    def close(self):
        if self.h:
            self.L.sd_screen_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_ms(self, reset=False):
        """Device time of the kernels of the calls so far whose keys came back to the host (ms)."""
        return float(self.L.sd_screen_kernel_ms(self.h, 1 if reset else 0))

    def kernel_bench(self, warmup=2, reps=5):
        """(screen_ms, dist_ms): the screen's launch beside the --ed_thr distance kernel alone on the batch of the last
        chunks() call with host reads, alternating, each between two HIP events (sd_screen_kernel_bench)."""
        a, b = (C.c_float * reps)(), (C.c_float * reps)()
        self._check(self.L.sd_screen_kernel_bench(self.h, int(warmup), int(reps), a, b, self._err, 4096))
        return list(a), list(b)

    def kernel(self):
        """The instantiation a call launches, named as tests/prefilter_cases.kernel_of names it."""
        w = C.c_int32()
        k = self.L.sd_screen_kernel(self.h, C.byref(w))
        return "sd_hw_dist<%d>" % w.value if k == 0 else "sd_hw_dist_u<%d,%s>" % (w.value, "hi" if k == 2 else "lo")

    def chunks(self, reads, part_size=5000, overlap=500, stream=None, device_out=False):
        """-> ScreenKeys of the reads: a read list, a ReadSet, or a DeviceReads (packed on the device, ordered behind
        reads.stream -- or `stream` -- by events; the buffer is free for later work on that stream when this returns).
        device_out=True (DeviceReads only): key stays on the device as an int32 torch tensor, written in order with
        that stream and without a host-side wait."""
        import numpy as np
        n = C.c_int64()
        if isinstance(reads, DeviceReads):
            cr, co, cl = chunk_table(reads.read_lens, part_size, overlap)
            st = reads.stream if stream is None else (stream if isinstance(stream, int) else int(stream.cuda_stream))
            if device_out:
                import torch
                dev = torch.device("cuda", reads.device)
                with torch.cuda.stream(_torch_stream(torch, dev, st)):
                    key = torch.empty(max(len(cr), 1), dtype=torch.int32, device=dev)
                kp, cap = C.c_void_p(key.data_ptr()), key.numel()
            else:
                key = np.zeros(max(len(cr), 1), dtype=np.uint32)
                kp, cap = C.c_void_p(key.ctypes.data), len(key)
            self._check(self.L.sd_screen_chunks_dev(self.h, C.c_void_p(reads.ptr), reads.c_off, reads.c_lens, reads.n,
                                                    int(part_size), int(overlap), C.c_void_p(st), kp, cap, C.byref(n),
                                                    self._err, 4096))
            assert n.value == len(cr)
            return ScreenKeys(cr, co, cl, key[:len(cr)])
        if device_out:
            raise SdError(SD_ERR_PARAM, "Screener.chunks: device_out needs reads in device memory (a DeviceReads)")
        rs = reads if isinstance(reads, ReadSet) else ReadSet(reads)
        cr, co, cl = chunk_table([len(s) for s in rs.seqs], part_size, overlap)
        key = np.zeros(max(len(cr), 1), dtype=np.uint32)
        self._check(self.L.sd_screen_chunks(self.h, rs.ptrs, rs.lens, rs.n, int(part_size), int(overlap), key.ctypes.data,
                                            len(key), C.byref(n), self._err, 4096))
        assert n.value == len(cr)
        return ScreenKeys(cr, co, cl, key[:len(cr)])


def screen_regions(keys, read_lens, thr, part_size=5000, overlap=500):
    """The regions of a threshold (sd_screen_regions, host only): a maximal run a..b of consecutive chunks of one read
    with key >> 16 <= thr is the bytes [a * part_size, min(len, (b + 1) * part_size + overlap)) of that read.  keys: a
    ScreenKeys (a device key is copied to the host: 4 bytes per chunk).  -> structured array (screen_region_dtype()):
    read, start, end_incl, n_chunks, best_key, in read order, then position order."""
    import numpy as np
    L = load()
    key = keys.key
    if hasattr(key, "cpu"):
        key = key.cpu().numpy().view(np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    cr = np.ascontiguousarray(keys.chunk_read, dtype=np.int32)
    if len(cr) != len(key):
        raise SdError(SD_ERR_PARAM, "screen_regions: %d keys for %d chunks" % (len(key), len(cr)))
    lens = np.ascontiguousarray(read_lens, dtype=np.int64)
    out = np.zeros(max(len(key), 1), dtype=screen_region_dtype())
    n = C.c_int64()
    err = C.create_string_buffer(4096)
    rc = L.sd_screen_regions(key.ctypes.data, cr.ctypes.data, len(key), lens.ctypes.data, len(lens), int(part_size),
                             int(overlap), int(thr), out.ctypes.data, len(out), C.byref(n), err, 4096)
    if rc != SD_OK:
        raise SdError(rc, err.value.decode(errors="replace"))
    return out[:n.value].copy()


def region_reads(reads, regions):
    """The regions as reads of their own, without moving a base: for a read list memoryview slices of the parents' bytes,
    for a DeviceReads a DeviceReads on the same buffer and stream with the regions' offsets and lengths."""
    if isinstance(reads, DeviceReads):
        off = [reads.read_off[int(g["read"])] + int(g["start"]) for g in regions]
        lens = [int(g["end_incl"]) - int(g["start"]) + 1 for g in regions]
        return DeviceReads(_KeepAlive((reads.ptr, reads.nbytes, reads.device), reads.data), lens, offsets=off,
                           stream=reads.stream)
    seqs = reads.seqs if isinstance(reads, ReadSet) else [_b(s) for s in reads]
    return [memoryview(seqs[int(g["read"])])[int(g["start"]):int(g["end_incl"]) + 1] for g in regions]


class _KeepAlive(tuple):
    """DeviceReads' (ptr, nbytes, device) form of a buffer, with the object that owns it kept alive."""

    def __new__(cls, t, keep):
        self = super().__new__(cls, t)
        self.keep = keep
        return self


def rows_from_regions(rows, row_off, regions, n_reads):
    """Rows of a job whose reads were regions (region_reads) -> rows of the parent reads: starts and ends shifted by
    the region's start, row_off rebuilt per parent read (n_reads + 1).  Host rows: a structured array with start / end
    fields (final_dtype() rows also get their read index mapped back) or an int32 [n, 4] array (tmpl, start, end, score),
    with a numpy row_off -> (rows, row_off).  A DeviceRows or DeviceFinalRows (row_off ignored): torch ops on its device
    -> the same type."""
    import numpy as np
    g_read = np.ascontiguousarray(regions["read"], dtype=np.int64)
    g_start = np.ascontiguousarray(regions["start"], dtype=np.int64)
    if isinstance(rows, (DeviceRows, DeviceFinalRows)):
        import torch
        dr = rows
        dev = dr.rows.device
        off = dr.row_off.to(torch.int64)
        cnt = off[1:] - off[:-1]
        shift = torch.repeat_interleave(torch.as_tensor(g_start, device=dev), cnt)
        per_read = torch.zeros(n_reads, dtype=torch.int64, device=dev)
        if len(g_read):
            per_read.index_add_(0, torch.as_tensor(g_read, device=dev), cnt)
        new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per_read, 0)])
        out = dr.rows.clone()
        if isinstance(dr, DeviceRows):
            out[:, 1:3] += shift.to(torch.int32)[:, None]
            return DeviceRows(out, new_off, dr.n_rows)
        w = out.view(torch.int64)            # sd_final_row: read (int32) at 0, start at 8, end at 16
        w[:, 1:3] += shift[:, None]
        rd = torch.repeat_interleave(torch.as_tensor(g_read, device=dev), cnt).to(torch.int32)
        out.view(torch.int32)[:, 0] = rd
        return DeviceFinalRows(out, new_off, dr.alt, dr.n_rows)
    off = np.ascontiguousarray(row_off, dtype=np.int64)
    if len(off) != len(g_read) + 1:
        raise SdError(SD_ERR_PARAM, "rows_from_regions: row_off has %d entries for %d regions" % (len(off), len(g_read)))
    cnt = off[1:] - off[:-1]
    shift = np.repeat(g_start, cnt)
    out = np.array(rows, copy=True)
    if out.dtype.names:
        out["start"] += shift.astype(out.dtype["start"])
        out["end"] += shift.astype(out.dtype["end"])
        if "read" in out.dtype.names:
            out["read"] = np.repeat(g_read, cnt)
    else:
        out = out.reshape(-1, 4)
        out[:, 1:3] += shift.astype(out.dtype)[:, None]
    per_read = np.bincount(g_read, weights=cnt, minlength=n_reads).astype(np.int64) if len(g_read) else np.zeros(n_reads, dtype=np.int64)
    return out, np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
