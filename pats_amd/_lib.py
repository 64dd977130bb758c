"""Loads libpats_amd.so (the C-ABI of include/pats_amd.h) with ctypes.

There is NO fallback: if the HIP library is missing or a call fails, this raises.  Nothing under
oracle/ is ever imported from here.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpats_amd.so")
# PATS_AMD_DIAG_LIB=1 (profiling tools only): the diagnostic twin with every third-level sweep variant and the timing
# ablations (`python -m pats_amd.build --diag`).  The production library refuses those variants.
if os.environ.get("PATS_AMD_DIAG_LIB", "") not in ("", "0"):
    _sfx = os.environ["PATS_AMD_DIAG_LIB"]
    LIB_PATH = os.path.join(_HERE, "libpats_amd_diag%s.so" % ("" if _sfx == "1" else _sfx))

c_void_p, c_int, c_i64, c_f, c_size = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                                       ctypes.c_size_t)

ABI_VERSION = 8      # include/pats_amd.h PATS_ABI_VERSION



class PairTable(ctypes.Structure):
    """pats_pair_table_t (include/pats_amd.h): the shapes of a ragged batch, host copies + device arrays."""
    _fields_ = [("pairs", ctypes.c_int64), ("shape_host", c_void_p), ("cell_base_host", c_void_p), ("shape", c_void_p),
                ("cell_base", c_void_p), ("img_base", c_void_p)]


_TAB = ctypes.POINTER(PairTable)


class CropFormat(ctypes.Structure):
    """pats_crop_format_t (include/pats_amd.h): the crops' dtype (pats_img_dtype_t), layout (0 hwc, 1 chw), normalisation."""
    _fields_ = [("dtype", ctypes.c_int32), ("layout", ctypes.c_int32), ("normalize", ctypes.c_int32),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


_FMT = ctypes.POINTER(CropFormat)

# the 22 arguments of a fixed-budget score entry, and what an adaptive one appends to them
_SCORE_ARGS = [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_int, c_f,
               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]
_ADAPTIVE_ARGS = [ctypes.c_double, c_int, c_int, c_i64, c_void_p, c_void_p]
_POLISH_ARGS = [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_int, c_f, c_void_p, c_i64,
                c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]

# name -> (restype, argtypes); must list every symbol include/pats_amd.h declares
SIGNATURES = {
    "pats_version": (ctypes.c_char_p, []),
    "pats_abi_version": (c_int, []),
    "pats_last_error": (ctypes.c_char_p, []),
    "pats_device_count": (c_int, []),
    "pats_set_sinkhorn_mode": (c_int, [c_int]),
    "pats_set_fine_fused": (c_int, [c_int]),
    "pats_set_third_gather": (c_int, [c_int]),
    "pats_sinkhorn_fallbacks": (c_int, [ctypes.POINTER(ctypes.c_int64), c_int]),
    "pats_sinkhorn_tail_solves": (c_int, [ctypes.POINTER(ctypes.c_int64), c_int]),
    "pats_set_gnn_redo_mode": (c_int, [c_int]),
    "pats_gnn_overflows": (c_int, [ctypes.POINTER(ctypes.c_int64), c_int]),
    "pats_cost_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "pats_sinkhorn_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "pats_sinkhorn_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                  c_void_p, c_size, c_void_p]),
    "pats_ot_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "pats_log_optimal_transport_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                               c_void_p, c_void_p, c_size, c_void_p]),
    "pats_ot2_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "pats_log_optimal_transport2_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                                c_f, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_cost_ot_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                 c_void_p, c_int, c_f, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_cost_ot_flags_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_set_cost_ot_mid_event": (c_int, [c_void_p]),
    "pats_cost_ot_flags_counted_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                               c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_iterative_expand_counted_f32": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                                  c_int, c_int, c_f, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_fine_descriptors_counted_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_int,
                                                  c_void_p, c_void_p]),
    "pats_log_optimal_transport2_flags_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                                      c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_colmass_flags_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "pats_cost_ot_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int, c_int]),
    "pats_colmass_sqrt_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p]),
    "pats_dustbin_bias_inplace_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_f, c_void_p]),
    "pats_exp_f32": (c_int, [c_void_p, c_i64, c_void_p, c_void_p]),
    "pats_argmax_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "pats_iterative_expand_f32": (c_int, [c_void_p, c_int, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                          c_int, c_int, c_f, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_split_patches": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "pats_split_patches_device": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_compute_imgs_bounds_batch_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_left_crops_counted_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, c_int, c_int,
                                            c_void_p, c_void_p]),
    "pats_tensor_resize_hwc_counted_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p,
                                                   c_void_p, c_void_p, c_void_p]),
    "pats_compute_imgs_bounds_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    "pats_left_crops_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_int, c_int, c_void_p,
                                    c_void_p]),
    "pats_tensor_resize_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p,
                                       c_void_p, c_void_p]),
    "pats_tensor_resize_hwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64,
                                           c_void_p, c_void_p, c_void_p]),
    "pats_compute_result_f32": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "pats_compute_result_ws_f32": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_size, c_void_p]),
    "pats_fine_descriptors_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "pats_third_descriptors_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_third_level_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "pats_third_descriptors_counted_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_fine_descriptors_nhwc_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "pats_third_descriptors_nhwc_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_fine_descriptors_typed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_i64, c_void_p,
                                            c_void_p, c_void_p]),
    "pats_third_descriptors_typed": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # the two above with the output element type (pats_map_dtype_t) behind the output pointers
    "pats_fine_descriptors_typed_out": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_i64, c_void_p,
                                                c_void_p, c_int, c_void_p]),
    "pats_third_descriptors_typed_out": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                 c_void_p]),
    "pats_third_level_counted_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    # descriptors in any pats_map_dtype_t (0 float32, 1 float16, 2 bfloat16); outputs as the _f32 entries'
    "pats_cost_typed": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "pats_cost_ot_typed": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_int, c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_third_level_typed": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_chunk_rows_workspace_bytes": (c_size, [c_i64, c_int]),
    "pats_chunk_rows_device": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_int, c_i64] + [c_void_p] * 13 +
                               [c_size, c_void_p]),
    "pats_profile_marker": (c_int, [c_int, c_void_p]),
    "pats_stream_create_cu_mask": (c_int, [c_void_p, c_int, c_void_p]),
    "pats_stream_destroy": (c_int, [c_void_p]),
    "pats_merge_batch_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "pats_merge_patches_batch": (c_int, [c_int, c_int, c_i64, c_int, c_int, c_i64] + [c_void_p] * 7 + [c_int, c_void_p, c_void_p,
                                         c_size, c_void_p]),
    "pats_merge_patches_chunks": (c_int, [c_int, c_int, c_int, c_int, c_i64, c_int, c_int, c_i64, c_i64] + [c_void_p] * 7 +
                                  [c_int, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_chunk_fine_tail_workspace_bytes": (c_size, [c_i64, c_i64, c_int, c_int]),
    "pats_chunk_fine_tail_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_int, c_f, c_void_p, c_void_p, c_int, c_int, c_int,
                                         c_i64, c_int, c_int, c_i64] + [c_void_p] * 5 + [c_int] + [c_void_p] * 16 + [c_void_p, c_size, c_void_p]),
    "pats_chunk_third_tail_workspace_bytes": (c_size, [c_i64, c_int, c_int]),
    "pats_chunk_third_tail_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                          c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p] + [c_void_p] * 10 +
                                  [c_void_p, c_size, c_void_p]),
    "pats_get_result_chunks_f32": (c_int, [c_int, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p,
                                           ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_merge_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int]),
    "pats_merge_patches": (c_int, [c_int, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_size, c_void_p]),
    "pats_compact_workspace_bytes": (c_size, [c_i64]),
    "pats_third_inputs_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_i64, c_void_p,
                                      c_void_p, c_size, c_void_p]),
    "pats_refine_scatter_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_i64, c_void_p,
                                        c_void_p, c_void_p, c_size, c_void_p]),
    "pats_attention_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "pats_attentional_propagation_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int]),
    "pats_attentional_propagation_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_int, c_f,
                                                 c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_propagation_packed_bytes": (c_size, [c_int, c_int]),
    "pats_propagation_pack_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_size, c_void_p]),
    "pats_attentional_propagation_packed_f32": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                        c_int, c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_attentional_gnn_packed_workspace_bytes": (c_size, [c_i64, c_int, c_int, c_int]),
    "pats_attentional_gnn_packed_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                c_void_p, c_f, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_attentional_propagation_packed_counted_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_int, c_int, c_int, c_int,
                                                                c_void_p, c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_size,
                                                                c_void_p]),
    "pats_matches_by_pair_workspace_bytes": (c_size, [c_int, c_i64]),
    "pats_matches_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_matches_by_pair_summary_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64, c_int,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_chunk_rows_ragged": (c_int, [_TAB, c_void_p, c_int, c_int, c_i64] + [c_void_p] * 14 + [c_size, c_void_p]),
    "pats_compute_imgs_bounds_ragged_f32": (c_int, [_TAB] + [c_void_p] * 10 + [c_void_p]),
    "pats_left_crops_ragged_f32": (c_int, [_TAB, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p]),
    "pats_tensor_resize_hwc_ragged_f32": (c_int, [_TAB, c_void_p, c_int, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_left_crops_typed": (c_int, [_TAB, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p,
                                      _FMT, c_void_p, c_void_p]),
    "pats_tensor_resize_hwc_typed": (c_int, [_TAB, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, _FMT,
                                             c_void_p, c_void_p, c_void_p]),
    "pats_tensor_resize_typed": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p, _FMT, c_void_p,
                                         c_void_p, c_void_p]),
    "pats_merge_ragged_workspace_bytes": (c_size, [c_i64]),
    "pats_merge_patches_ragged": (c_int, [_TAB, c_int, c_int, c_i64] + [c_void_p] * 8 + [c_int, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_get_result_chunks_ragged_f32": (c_int, [_TAB, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p,
                                                  ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                                  c_void_p, c_void_p, c_size, c_void_p]),
    "pats_matches_by_row_pair_summary_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_i64,
                                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # the image front end (csrc/prepare.hip): the table in host and in device memory, n_img, left, left_elems, right, right_elems, dtype
    "pats_prepare_images_max_side": (c_i64, []),
    "pats_prepare_images_u8": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p]),
    # per-match confidence: the entries they are named after with the confidence pointer(s) added
    "pats_third_level_typed_conf": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "pats_compute_result_ws_conf_f32": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_size, c_void_p]),
    "pats_refine_scatter_conf_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_i64, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_get_result_chunks_conf_f32": (c_int, [c_int, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_get_result_chunks_ragged_conf_f32": (c_int, [_TAB, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                       ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_matches_by_pair_summary_conf_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                      c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_size, c_void_p]),
    "pats_matches_by_row_pair_summary_conf_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                          c_int, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                          c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair top-K over the regrouped matches (csrc/topk.hip)
    "pats_topk_by_pair_max_k": (c_i64, []),
    "pats_topk_by_pair_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_topk_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_f, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair spread top-K: one winner per image cell, the K most confident winners (csrc/topk_spread.hip)
    "pats_topk_spread_by_pair_max_cells": (c_i64, []),
    "pats_topk_spread_by_pair_workspace_bytes": (c_size, [c_i64, c_i64, c_i64, c_i64]),
    "pats_topk_spread_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_f, c_int, c_i64,
                                             c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_size, c_void_p]),
    # per-pair verification of candidate epipolar models (csrc/epipolar.hip)
    "pats_epipolar_max_h": (c_i64, []),
    "pats_epipolar_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_epipolar_score_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                                c_void_p, c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_size, c_void_p]),
    # per-pair 8-point hypotheses for that verification (csrc/hypotheses.hip)
    "pats_epipolar_hypotheses_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_epipolar_hypotheses_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair 5-point hypotheses: up to ten essential matrices per sample (csrc/hypotheses5.hip)
    "pats_epipolar_hypotheses5_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_epipolar_hypotheses5_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                      c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair relative pose from the verified inliers (csrc/pose.hip)
    "pats_epipolar_pose_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_epipolar_pose_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                               c_void_p, c_i64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair triangulation of the posed matches (csrc/triangulate.hip)
    "pats_epipolar_triangulate_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_epipolar_triangulate_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair pose error against the ground truth and the AUC over accumulated errors (csrc/pose_error.hip)
    "pats_pose_error_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, ctypes.c_double, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_pose_auc_max_n": (c_i64, []),
    "pats_pose_auc_f64": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p]),
    # per-pair homographies: 4-point hypotheses (csrc/hypotheses.hip), verification (csrc/epipolar.hip), refit (csrc/homography.hip)
    "pats_homography_hypotheses_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_homography_hypotheses_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                       c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_homography_score_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_homography_score_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                                  c_void_p, c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_size, c_void_p]),
    "pats_homography_refit_workspace_bytes": (c_size, [c_i64]),
    "pats_homography_refit_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    # per-pair pose from a verified homography and the per-pair E-or-H decision (csrc/pose_h.hip)
    "pats_homography_pose_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_homography_pose_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                                 c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double] + [c_void_p] * 14 +
                                         [c_void_p, c_size, c_void_p]),
    "pats_pose_select_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_pose_select_by_pair": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64] + [c_void_p] * 23 + [c_void_p, c_size, c_void_p]),
    # per-pair adaptive verification, both branches (csrc/adaptive.hip): the fixed-budget arguments, then confidence, sample_size,
    # models_per_sample, round_models, used, participating
    "pats_epipolar_score_adaptive_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_epipolar_score_adaptive_by_pair_f32": (c_int, _SCORE_ARGS + _ADAPTIVE_ARGS),
    "pats_homography_score_adaptive_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_homography_score_adaptive_by_pair_f32": (c_int, _SCORE_ARGS + _ADAPTIVE_ARGS),
    # per-pair MSAC scoring, both branches (csrc/epipolar.hip): the fixed-budget arguments, then gains, best_gain
    "pats_msac_gain_one": (c_i64, []),
    "pats_epipolar_score_msac_by_pair_f32": (c_int, _SCORE_ARGS + [c_void_p, c_void_p]),
    "pats_homography_score_msac_by_pair_f32": (c_int, _SCORE_ARGS + [c_void_p, c_void_p]),
    # per-pair local optimisation, both branches (csrc/polish.hip): the verification's match, segment, thr, norm and min_conf
    # arguments, then models, H, best, rounds, the six outputs, workspace, stream
    "pats_epipolar_polish_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_epipolar_polish_by_pair_f32": (c_int, _POLISH_ARGS),
    "pats_homography_polish_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_homography_polish_by_pair_f32": (c_int, _POLISH_ARGS),
    # the uncalibrated branch: 7-point hypotheses, up to three fundamental matrices per sample (csrc/hypotheses7.hip), the rank-2
    # refit (csrc/fundamental.hip: the homography refit's arguments with sigma and f_refit behind eig) and its local optimisation
    "pats_epipolar_hypotheses7_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_epipolar_hypotheses7_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                      c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_fundamental_refit_workspace_bytes": (c_size, [c_i64]),
    "pats_fundamental_refit_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size, c_void_p]),
    "pats_fundamental_polish_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_fundamental_polish_by_pair_f32": (c_int, _POLISH_ARGS),
    # the plane-and-parallax (DEGENSAC) stage of the uncalibrated branch (csrc/plane_parallax.hip): the 7-point generator's arguments
    # without progressive and n_models, then the plane (models_h, Mh, best_h, thr), parallax, models, sample_idx, pool; the hand-over:
    # the lists and segments, norm, the plane, the standing and the new verification (models, H, best, best_count, inlier, moments
    # each), then model, best_count, inlier, moments, replaced, overlap
    "pats_plane_parallax_pool_max": (c_i64, []),
    "pats_plane_parallax_hypotheses_workspace_bytes": (c_size, [c_i64, c_i64]),
    "pats_plane_parallax_hypotheses_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                           c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_f, c_void_p, c_void_p,
                                                           c_void_p, c_void_p, c_size, c_void_p]),
    "pats_plane_parallax_select_by_pair": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p,
                                                   c_void_p, c_i64, c_void_p, c_void_p,
                                                   c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # the absolute-pose branch (csrc/absolute.hip): the lift through a depth map, P3P hypotheses, reprojection verification
    "pats_lift_by_pair_f32": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_f,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_absolute_hypotheses_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_void_p,
                                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pats_absolute_score_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                                c_void_p, c_void_p, c_int, c_f, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # ... and its local optimisation: the verification's arguments up to min_conf, then best, rounds, steps, the six outputs, stream
    "pats_absolute_polish_by_pair_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                                 c_void_p, c_void_p, c_int, c_f, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    # per-pair match error against depth-and-pose ground truth (csrc/match_error.hip): the lists and conf, the segments, norm, T1, T0,
    # swapped, the right depth table, occl_rel, size_r, the gate, thr + n_thr and edges + B (host arrays), mask, the seven outputs, stream
    "pats_match_error_by_pair_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                             c_void_p, c_int, c_void_p, ctypes.c_double, c_void_p, c_int, c_f, c_void_p, c_i64, c_void_p,
                                             c_i64, c_void_p] + [c_void_p] * 7 + [c_void_p]),
    "pats_conv1x1_workspace_bytes": (c_size, []),
    "pats_conv1x1_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size, c_void_p]),
    "pats_bn_fold_workspace_bytes": (c_size, [c_int]),
    "pats_bn_fold_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_f, c_void_p, c_void_p, c_void_p,
                                 c_size, c_void_p]),
    "pats_scale_head_f32": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_void_p]),
    "pats_get_result_workspace_bytes": (c_size, [c_i64, c_i64, c_i64]),
    "pats_get_result_f32": (c_int, [c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                    ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_i64, c_void_p, c_void_p, c_size, c_void_p]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pats_amd: %s is missing - the HIP extension was not built (run "
                "`python -m pats_amd.build` / __graft_entry__.build()). There is no CPU fallback."
                % LIB_PATH)
        # PyTorch ships its own libamdhip64; if this library were loaded first it would bring in /opt/rocm's copy, torch
        # would then load its own beside it, and the kernels launched here would talk to a runtime that has no
        # device context ("no ROCm-capable device is detected" - seen when build() and smoke() ran in one process).
        # Loading torch's runtime first makes both resolve to the same one.
        try:
            import torch  # noqa: F401
        except ImportError:      # a C-ABI-only consumer without torch: nothing to clash with
            pass
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)     # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.pats_abi_version() != ABI_VERSION:
            raise ImportError("pats_amd: %s exports ABI %d, these bindings were written for ABI %d - rebuild the library "
                              "(python -m pats_amd.build)" % (LIB_PATH, handle.pats_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().pats_last_error().decode()
        raise RuntimeError("pats_amd.%s failed (code %d): %s" % (what, rc, msg))
