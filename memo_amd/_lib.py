"""ctypes binding of the C ABI declared in include/memo_amd.h, memo_amd_multi.h, memo_amd_dap.h and
memo_amd_transport.h.

There is NO fallback: if libmemo_amd.so is missing or a HIP call fails, this raises.
The CPU restatement under oracle/ is test infrastructure and is never imported here.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("MEMO_AMD_LIB") or os.path.join(_HERE, "libmemo_amd.so")   # override: A/B of builds
# the product objects + the A/B switches of include/memo_amd_debug.h (tests, fuzzers, tools/ab.py)
AB_SO_PATH = os.environ.get("MEMO_AMD_AB_LIB") or os.path.join(_HERE, "libmemo_amd_ab.so")

MEMO_OK, MEMO_EINVAL, MEMO_EHIP, MEMO_ENOTREADY, MEMO_EUNSORTED, MEMO_ELONGROW, MEMO_EUNPACKABLE = 0, -1, -2, -3, -4, -5, -6


class MemoError(RuntimeError):
    """A C-ABI call returned a negative code (message from memo_last_error())."""

    def __init__(self, code, msg):
        super().__init__(f"memo_amd error {code}: {msg}")
        self.code = code


class MemoIndexError(MemoError, IndexError):
    """The reference raises IndexError here (annot column outside the result matrix)."""


class MemoValueError(MemoError, ValueError):
    """The reference raises ValueError here (window end before window start)."""


class MemoUnpackable(MemoError):
    """memo_builder_*: the rows cannot take the packed way in; upload them as int64 columns."""


class IndexInfo(C.Structure):
    """memo_index_info_t (include/memo_amd.h): versioned -- set struct_bytes before memo_index_get_info_v5"""
    _fields_ = [("struct_bytes", C.c_uint32), ("version", C.c_uint32),
                ("rows", C.c_uint64), ("min_start", C.c_int64), ("max_start", C.c_int64),
                ("device", C.c_int32), ("bucket_shift", C.c_int32), ("buckets", C.c_uint64),
                ("was_sorted", C.c_int32), ("finalized", C.c_int32), ("device_bytes", C.c_uint64),
                ("packed_format", C.c_int32), ("has_wide", C.c_int32), ("pack_ms", C.c_float),
                ("dense_rows", C.c_int32), ("long_rows", C.c_uint64), ("max_annot", C.c_uint64),
                ("bucket_base", C.c_int64), ("last_sweep", C.c_int32), ("last_variant", C.c_int32), ("dense_row_count", C.c_uint64), ("last_rows_read", C.c_uint64),
                ("last_view_ms", C.c_float), ("row_order", C.c_int32), ("side_bytes", C.c_uint64),
                ("views_resident", C.c_int32), ("tile_tables_resident", C.c_int32), ("view_builds", C.c_uint64),
                ("last_level_arrays", C.c_int32), ("last_view_placed", C.c_int32), ("view_placings", C.c_uint64),
                ("last_view_rows_per_group", C.c_int32), ("last_tile_width", C.c_int32)]


class MsLayoutInfo(C.Structure):
    """memo_ms_layout_info_t (include/memo_amd_dap.h)"""
    _fields_ = [("layout", C.c_int32), ("block", C.c_int32), ("device_bytes", C.c_uint64), ("dense_bytes", C.c_uint64),
                ("flagged", C.c_uint64), ("encode_ms", C.c_float), ("decode_ms", C.c_float)]


class MsWalkInfo(C.Structure):
    """memo_ms_walk_info_t (include/memo_amd_dap.h)"""
    _fields_ = [("text_reads", C.c_uint64), ("max_chunk_text_reads", C.c_uint64), ("seeds", C.c_uint64),
                ("seed_text_reads", C.c_uint64), ("budget", C.c_int64)]


# every symbol the product headers declare: name -> (restype, argtypes)
_P, _I32, _I64, _U64, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t
SYMBOLS = {
    "memo_last_error": (C.c_char_p, []),
    "memo_device_count": (C.c_int, []),
    "memo_version": (C.c_char_p, []),
    "memo_host_threads": (C.c_int, [C.POINTER(_I32), C.POINTER(C.c_double)]),
    "memo_index_create": (C.c_int, [_U64, _I32, C.POINTER(_P)]),
    "memo_index_upload": (C.c_int, [_P, _P, _P, _P, _U64]),
    "memo_index_upload_rows": (C.c_int, [_P, _U64, _P, _P, _P, _U64]),
    "memo_index_truncate": (C.c_int, [_P, _U64]),
    "memo_index_columns": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "memo_index_finalize": (C.c_int, [_P, _I32, _I32]),
    "memo_index_pack": (C.c_int, [_P, _I32]),
    "memo_index_pack_dense": (C.c_int, [_P, _I32]),
    "memo_index_get_info_v5": (C.c_int, [_P, C.POINTER(IndexInfo)]),
    "memo_index_set_option": (C.c_int, [_P, _I32, _I64]),
    "memo_index_prepare": (C.c_int, [_P, _I32, _I32, _I32, _I64, _P, C.POINTER(_U64)]),
    "memo_index_export_packed": (C.c_int, [_P, _P, _P, _P, _P]),
    "memo_index_import_packed": (C.c_int, [_U64, _I32, _I32, _I64, _P, _P, _P, _U64, _I64, _I64, _I64, _U64, _P, _U64,
                                           C.POINTER(_P)]),
    "memo_index_export_dense": (C.c_int, [_P, _P, _P, _P]),
    "memo_index_export_view": (C.c_int, [_P, _I32, _I32, _P, _P, _P, _P, _P]),
    "memo_index_import_dense": (C.c_int, [_U64, _I32, _I32, _I64, _P, _P, _U64, _I64, _I64, _I64, _U64, _P, _U64,
                                          C.POINTER(_P)]),
    "memo_dense_rows_can_answer": (C.c_int, [_U64, _I64, _I64, _U64, _I32, _I32, _I32]),
    "memo_index_destroy": (None, [_P]),
    "memo_builder_create": (C.c_int, [_U64, _I32, _I32, C.POINTER(_P)]),
    "memo_builder_create_rows": (C.c_int, [_U64, _I32, _I32, _I32, C.POINTER(_P)]),
    "memo_builder_push": (C.c_int, [_P, _P, _P, _P, _U64]),
    "memo_builder_push_rows": (C.c_int, [_P, _P, _U64]),
    "memo_builder_finish": (C.c_int, [_P, C.POINTER(_P)]),
    "memo_builder_destroy": (None, [_P]),
    "memo_query_conservation_dev": (C.c_int, [_P, _I64, _I64, _I32, _I32, _P, _P]),
    "memo_query_membership_dev": (C.c_int, [_P, _I64, _I64, _I32, _I32, _P, _P]),
    "memo_query_conservation_u8_dev": (C.c_int, [_P, _I64, _I64, _I32, _I32, _P, _P]),
    "memo_query_check": (C.c_int, [_P, _P]),
    "memo_conservation": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I32, _I32, _P, _I32]),
    "memo_membership": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I32, _I32, _P, _I32]),
    "memo_conservation_rows": (C.c_int, [_P, _U64, _I64, _I64, _I32, _I32, _P, _I32]),
    "memo_membership_rows": (C.c_int, [_P, _U64, _I64, _I64, _I32, _I32, _P, _I32]),
    "memo_split_window": (C.c_int, [_I64, _I64, _I32, _I32, C.c_double, _P]),
    "memo_conservation_multi": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I32, _I32, _P, _P, _I32]),
    "memo_membership_multi": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I32, _I32, _P, _P, _I32]),
    "memo_query_conservation_multi_dev": (C.c_int, [_P, _I32, _I64, _I64, _I32, _I32, _P, _I32, _P, C.c_double]),
    "memo_query_membership_multi_dev": (C.c_int, [_P, _I32, _I64, _I64, _I32, _I32, _P, _I32, _P, C.c_double]),
    "memo_dev_malloc": (C.c_int, [_I32, _SZ, C.POINTER(_P)]),
    "memo_dev_free": (C.c_int, [_I32, _P]),
    "memo_dev_upload": (C.c_int, [_I32, _P, _P, _SZ, _P]),
    "memo_dev_download": (C.c_int, [_I32, _P, _P, _SZ, _P]),
    "memo_emit_conservation": (_SZ, [_P, _I64, _P, _SZ]),
    "memo_emit_membership": (_SZ, [_P, _I64, _I32, _P, _SZ]),
    "memo_bin_conservation_dev": (C.c_int, [_P, _I64, _P, _I32, _I32, _P, _I32, _P]),
    "memo_runs_conservation_dev": (C.c_int, [_P, _I64, _I32, _I32, _I32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_U64), _I32, _P]),
    "memo_runs_membership_dev": (C.c_int, [_P, _I64, _I32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_U64), _I32, _P]),
    "memo_runs_tile": (_I32, [_I32]),
    "memo_cooccurrence_dev": (C.c_int, [_P, _I64, _I32, _P, _I32, _P]),
    "memo_cooccurrence_tile": (_I32, [_I32]),
    "memo_query_membership_slice_dev": (C.c_int, [_P, _I64, _I64, _I64, _I64, _I32, _I32, _P, _P]),
    "memo_collect_dev": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _P, _P, _I32, _P]),
    "memo_collect_tile": (_I32, [_I32]),
    "memo_panel_planes_dev": (C.c_int, [_P, _I64, _I32, _P, _I64, _I64, _I32, _P]),
    "memo_panel_begin_dev": (C.c_int, [_P, _I64, _I32, _I64, _P, _P, _I32, _P]),
    "memo_panel_score_dev": (C.c_int, [_P, _I64, _I32, _I64, _P, _P, _P, _I32, _P, _I32, _P]),
    "memo_panel_take_dev": (C.c_int, [_P, _I64, _I32, _I64, _I32, _P, _P, _P, _I32, _P]),
    "memo_panel_tile": (_I32, []),
    "memo_panel_pass_words": (_I32, []),
    "memo_cover_weights_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _P, _I32, _P, _I64, _I32, _I64, _I32, _P]),
    "memo_cover_begin_dev": (C.c_int, [_P, _I64, _I32, _I32, _I64, C.c_uint32, _P, _P, _I32, _P]),
    "memo_cover_score_dev": (C.c_int, [_P, _I64, _I32, _I32, _I64, _P, _P, _P, _I32, _P, _I32, _P]),
    "memo_cover_take_dev": (C.c_int, [_P, _I64, _I32, _I32, _I64, _I32, _P, _P, _P, _I32, _P]),
    "memo_cover_pass_cells": (_I32, [_I32]),
    "memo_tracks_dev": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _P, _I32, _P]),
    "memo_tracks_tile": (_I32, [_I32]),
    "memo_breaks_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _I32, _I64, _P, _I32, _P, _I32, _P]),
    "memo_breaks_tile": (_I32, []),
    "memo_pairs_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _P, _I32, _P]),
    "memo_pairs_tile": (_I32, []),
    "memo_pairs_chunk": (_I32, []),
    "memo_pairs_narrow_span": (C.c_uint32, []),
    "memo_nearest_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _P, _I64, _P, _I32, _P, _P, _P, _I32, _P]),
    "memo_nearest_tile": (_I32, [_I32]),
    "memo_mosaic_fold_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _P, _P, _P, _I32, _P]),
    "memo_mosaic_parse_dev": (C.c_int, [_P, _P, _I64, C.POINTER(_P), C.POINTER(_P), C.POINTER(_U64), _I32, _P]),
    "memo_mosaic_tile": (_I32, []),
    "memo_segment_conservation_dev": (C.c_int, [_P, _I64, _I64, _P, _I32, _I32, _P, _I32, _P]),
    "memo_segment_conservation_tile": (_I32, []),
    "memo_feature_sums_dev": (C.c_int, [_P, _I32, _I32, _P, _P, _I32, _P, _I32, _P]),
    "memo_feature_sums_tile": (_I32, []),
    "memo_maxk_begin_dev": (C.c_int, [_P, _I64, C.c_uint32, _I32, _P]),
    "memo_maxk_rows_dev": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, C.c_uint32, _I32, _I64, _P, _I32, _P]),
    "memo_maxk_finish_dev": (C.c_int, [_P, _I64, C.c_uint32, _I32, _P]),
    "memo_maxk_tile": (_I32, []),
    "memo_emit_u32": (_SZ, [_P, _I64, _P, _SZ]),
    "memo_lengths_begin_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, _I64, _P, _I32, _P]),
    "memo_lengths_rows_dev": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I64, _I32, C.c_uint32, _P, _I32, _P]),
    "memo_lengths_carry_dev": (C.c_int, [_P, _P, _P, _U64, _I64, _I64, _I32, _P, _I32, _P]),
    "memo_lengths_finish_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, _I32, _P]),
    "memo_lengths_select_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, _I32, _P, _I32, _P]),
    "memo_lengths_tile": (_I32, []),
    "memo_lengths_select_tile": (_I32, [_I32]),
    "memo_mems_dev": (C.c_int, [_P, _I64, _I64, _I32, C.c_uint32, C.c_uint32, _I32, _I32, C.POINTER(_P), C.POINTER(_P), _P, _I32, _P]),
    "memo_mems_tile": (_I32, []),
    "memo_emit_intervals": (_SZ, [C.c_char_p, _P, _P, _P, _U64, _P, _SZ]),
    "memo_spectrum_scratch_bytes": (_SZ, [_I32, _I32]),
    "memo_spectrum_begin_dev": (C.c_int, [_P, _I32, _I32, _I32, _P]),
    "memo_spectrum_add_dev": (C.c_int, [_P, _I64, _I64, _I32, _I32, _I32, _P, _I32, _P]),
    "memo_spectrum_finish_dev": (C.c_int, [_P, _I32, _I32, _P, _I32, _P]),
    "memo_spectrum_tile": (_I32, [_I32, _I32, _I32]),
    "memo_convert_dap_dev": (C.c_int, [_P, _I64, _I32, _I64, _I64, _I64, _P, _I32, _P]),
    "memo_convert_tile": (_I32, []),
    "memo_add_dap_dev": (C.c_int, [_P, _I64, _I32, _I64, _I64, _I64, _P, _I32, _P, _I32, _P]),
    "memo_add_tile": (_I32, []),
    "memo_merge_dap_dev": (C.c_int, [_P, _I64, _I32, _P, _I32, _I64, _I64, _I64, _P, _I32, _P]),
    "memo_merge_tile": (_I32, []),
    "memo_emit_u32_rows": (_SZ, [_P, _I64, _I64, _I32, _P, _SZ]),
    "memo_emit_u32_rows_threads": (_I32, [_I64, _I32]),
    "memo_emit_runs": (_SZ, [C.c_char_p, _I64, _I64, _P, _P, _U64, _P, _SZ]),
    "memo_emit_membership_runs": (_SZ, [C.c_char_p, _I64, _I64, _P, _P, _U64, _I32, _P, _SZ]),
    "memo_parse_conservation_text_dev": (C.c_int, [_P, _I64, _P, _I64, C.POINTER(_I64), C.POINTER(_I64), _I32, _P]),
    "memo_dev_upload_pipelined": (C.c_int, [_I32, _P, _P, _SZ]),
    "memo_dap_create": (C.c_int, [_I32, _P, _I32, _I32, _I32, _I32, C.POINTER(_P)]),
    "memo_dap_push": (C.c_int, [_P, _P, _I64, C.POINTER(_U64)]),
    "memo_dap_fetch": (C.c_int, [_P, _P, _P, _P, _P]),
    "memo_dap_finish": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(_U64)]),
    "memo_dap_push_dev": (C.c_int, [_P, _P, _I64, C.POINTER(_U64)]),
    "memo_dap_destroy": (None, [_P]),
    "memo_ms_create": (C.c_int, [_P, _P, _I32, _I32, _I64, _I32, C.POINTER(_P)]),
    "memo_ms_create_layout": (C.c_int, [_P, _P, _I32, _I32, _I64, _I32, _I32, C.POINTER(_P)]),
    "memo_ms_plan_layout": (C.c_int, [_I64, _I32, _U64, _I32, C.POINTER(_I32), C.POINTER(_I64)]),
    "memo_ms_layout_info": (C.c_int, [_P, C.POINTER(MsLayoutInfo)]),
    "memo_ms_column_info": (C.c_int, [_P, _I32, C.POINTER(_U64), C.POINTER(_U64)]),
    "memo_ms_add_genome": (C.c_int, [_P, _P, _I64, _I32]),
    "memo_ms_add_records": (C.c_int, [_P, _P, _P, _I32, _I32, _I64, C.POINTER(_I32)]),
    "memo_ms_plan_pieces": (C.c_int, [_P, _I32, _I64, _P, C.POINTER(_I32)]),
    "memo_ms_fetch": (C.c_int, [_P, _I64, _I64, _P]),
    "memo_ms_push_dap": (C.c_int, [_P, _P, _I64, _I64, C.POINTER(_U64)]),
    "memo_ms_rows_dev": (C.c_int, [_P, _I64, _I64, C.POINTER(_P)]),
    "memo_ms_timings": (C.c_int, [_P, _P]),
    "memo_ms_set_walk_budget": (C.c_int, [_P, _I64]),
    "memo_ms_walk_info": (C.c_int, [_P, C.POINTER(MsWalkInfo)]),
    "memo_ms_destroy": (None, [_P]),
    "memo_suffix_array": (C.c_int, [_P, _I64, _P, _I32]),
    "memo_parse_ints": (C.c_int64, [_P, _SZ, _P, _SZ]),
    "memo_emit_bed": (_SZ, [_P, _P, _P, _P, _U64, _P, _I32, _P, _SZ]),
    "memo_transport_runs_bytes": (_SZ, [_I64, C.c_uint32]),
    "memo_transport_runs_pack_dev": (C.c_int, [_P, _I64, C.c_uint32, _P, _I32, _P]),
    "memo_transport_runs_unpack_dev": (C.c_int, [_P, _I64, C.c_uint32, _P, _I32, _P]),
    "memo_transport_runs_stats": (C.c_int, [_P, _I32, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "memo_transport_runs16_pack_dev": (C.c_int, [_P, _I64, C.c_uint32, _P, _I32, _P]),
    "memo_transport_runs16_unpack_dev": (C.c_int, [_P, _I64, C.c_uint32, _P, _I32, _P]),
    "memo_transport_runs_unpack_many_dev": (C.c_int, [_P, _P, _I32, _I64, C.c_uint32, _I32, _I32, _P]),
    "memo_transport_bytes": (_SZ, [_I64, C.c_uint32]),
    "memo_transport_pack_dev": (C.c_int, [_P, _I64, C.c_uint32, _P, _I32, _P]),
    "memo_transport_unpack_dev": (C.c_int, [_P, _I64, _P, _I32, _P]),
    "memo_transport_exceptions": (C.c_int, [_P, _I32, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "memo_transport_dense_bytes": (_SZ, [_I64, C.c_uint32, C.c_uint32]),
    "memo_transport_dense_pack_dev": (C.c_int, [_P, _I64, C.c_uint32, C.c_uint32, _P, _I32, _P]),
    "memo_transport_dense_unpack_dev": (C.c_int, [_P, _I64, C.c_uint32, C.c_uint32, _P, _I32, _P]),
    "memo_transport_dense_stats": (C.c_int, [_P, _I32, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "memo_synth_fill": (C.c_int, [_P, _U64, _U64, _U64, _I32, _U64]),
}

# include/memo_amd_debug.h: exported by libmemo_amd_ab.so only
DEBUG_SYMBOLS = {
    "memo_debug_set_tuning": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32]),
    "memo_debug_stream_rows": (C.c_int, [_P, _P]),
    "memo_debug_row_order": (C.c_int, [_P, _I32]),
    "memo_debug_no_views": (C.c_int, [_P, _I32]),
    "memo_debug_view_colouring": (C.c_int, [_I32]),
    "memo_debug_six_views": (C.c_int, [_I32]),
    "memo_debug_view_live": (C.c_int, [_P, _I32, C.POINTER(_U64)]),
    "memo_debug_view_deciding": (C.c_int, [_P, _I32, C.POINTER(_U64)]),
    "memo_debug_export_deciding": (C.c_int, [_P, _I32, _P, _P, _P, _P]),
    "memo_debug_view_runs": (C.c_int, [_P, _I32, C.POINTER(_U64)]),
    "memo_debug_export_runs": (C.c_int, [_P, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "memo_debug_fail_side_allocations": (C.c_int, [_I32]),
    "memo_debug_dense_keep_all": (C.c_int, [_I32]),
    "memo_debug_one_shot_way": (C.c_int, [_I32]),
    "memo_debug_last_one_shot_sweep": (C.c_int, []),
    "memo_debug_last_membership": (C.c_int, [_P, C.POINTER(_I32)]),
    "memo_debug_last_tiles_per_group": (C.c_int, [_P, C.POINTER(_I32)]),
    "memo_debug_last_pick": (C.c_int, [_P, C.POINTER(_I32), _I32]),
    "memo_debug_set_stamp_buffer":(C.c_int, [_P]),
    "memo_debug_ms_free_bytes": (C.c_int, [_I64]),
    "memo_debug_cooc_flush": (C.c_int, [_I32]),
    "memo_debug_cooc_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_tracks_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_breaks_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_pairs_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_nearest_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_nearest_lds": (C.c_int, [_I32]),
    "memo_debug_mosaic_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_mosaic_shape": (C.c_int, [_I32, _I32]),
    "memo_debug_features_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_maxk_rows": (C.c_int, [_I32]),
    "memo_debug_maxk_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_collect_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_panel_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_cover_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_lengths_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_spectrum_times": (C.c_int, [_I32, C.POINTER(C.c_float), C.POINTER(_I32), C.POINTER(_U64)]),
    "memo_debug_mems_times": (C.c_int, [_I32, C.POINTER(C.c_float)]),
    "memo_debug_ms_piece_text": (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _P, _I64, C.POINTER(_I64)]),
}


def build(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "-s", "clean"])
    subprocess.check_call(["make", "-C", src, "-s", "-j", str(min(4, os.cpu_count() or 1))])
    return SO_PATH


_lib = None
_product = None
_ab = None


def _bind(path, symbols):
    L = C.CDLL(path)
    for name, (res, args) in symbols.items():
        f = getattr(L, name)        # AttributeError if the library does not export it
        f.restype = res
        f.argtypes = args
    return L


def use_ab(on=True):
    """Make lib() hand out libmemo_amd_ab.so (product objects + the A/B switches) instead of the
    product library -- for tests and tools that set kernel shapes.  Returns the library now in use."""
    global _lib, _ab
    lib()
    if on:
        if _ab is None:
            if not os.path.exists(AB_SO_PATH):
                build()
            _ab = _bind(AB_SO_PATH, {**SYMBOLS, **DEBUG_SYMBOLS})
        _lib = _ab
    else:
        _lib = _product
    return _lib


def lib():
    global _lib, _product
    if _lib is None:
        if not os.path.exists(SO_PATH) and not os.environ.get("MEMO_AMD_LIB"):
            try:                                  # compile the real thing; never substitute for it
                build()
            except Exception:
                pass
        if not os.path.exists(SO_PATH):
            raise ImportError(f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                              "g.build()'` or `make -C memo_amd/csrc` -- there is no CPU fallback")
        _product = _lib = _bind(SO_PATH, SYMBOLS)
    return _lib


def check(rc):
    if rc < 0:
        msg = lib().memo_last_error().decode(errors="replace")
        if rc == MEMO_EINVAL and "IndexError" in msg:
            raise MemoIndexError(rc, msg)
        if rc == MEMO_EINVAL and "ValueError" in msg:
            raise MemoValueError(rc, msg)
        if rc == MEMO_EUNPACKABLE:
            raise MemoUnpackable(rc, msg)
        raise MemoError(rc, msg)
    return rc
