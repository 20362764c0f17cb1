"""ctypes loader of libusip_hip.so -- the only way the product reaches its kernels.

There is no fallback: if the library is missing or fails to load, every operator raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# USIP_LIB=<path>: load another BUILD of the same library (same-box A/B of two builds, tools/ab_build.sh); never a fallback
LIB_PATH = os.environ.get("USIP_LIB") or os.path.join(_HERE, "libusip_hip.so")
ABI = 6                      # = "abi=<n>" of usip_version(): bumped with every incompatible change of include/usip_hip.h
_lib = None

_f32p = ctypes.c_void_p
_i32p = ctypes.c_void_p
_int = ctypes.c_int
_flt = ctypes.c_float
_dbl = ctypes.c_double
_stream = ctypes.c_void_p

# name -> argtypes; must list every symbol include/usip_hip.h declares (tests check this).
SIGNATURES = {
    "usip_version": ([], ctypes.c_char_p),
    "usip_set_tuning": ([ctypes.c_char_p, _int], _int),
    "usip_tuning_value": ([_int], _int),
    "usip_launch_log": ([_int], _int),
    "usip_launch_log_entry": ([_int, ctypes.POINTER(ctypes.c_uint)], ctypes.c_char_p),
    "usip_wgrad_defer": ([_int], _int),
    "usip_wgrad_defer_on": ([_stream], _int),
    "usip_wgrad_defer_hold": ([_int], _int),
    "usip_wgrad_flush": ([_stream], _int),
    "usip_index_max_f32": ([_f32p, _i32p, _i32p, _int, _int, _int, _int, _stream], _int),
    "usip_index_max_geometry": ([_int, _int, _int, _int] + [ctypes.POINTER(_int)] * 3, _int),
    "usip_index_max_f32_cpu": ([_f32p, _i32p, _i32p, _int, _int, _int, _int, _int], _int),
    "usip_ball_query_f32": ([_f32p, _i32p, _flt, _int, _int, _int, _int, _stream], _int),
    "usip_ball_query_f32_cpu": ([_f32p, _i32p, _flt, _int, _int, _int, _int], _int),
    "usip_pairwise_dist_f32_cpu": ([_f32p, _f32p, _f32p, _int, _int, _int], _int),
    "usip_pairwise_dist_f32": ([_f32p, _f32p, _f32p, _int, _int, _int, _stream], _int),
    "usip_som_assign_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _stream], _int),
    "usip_som_cluster_f32": ([_f32p, _i32p, _f32p, _i32p, _f32p, _int, _int, _int, _stream], _int),
    "usip_som_cluster_csr_f32": ([_f32p, _i32p, _i32p, _i32p, _f32p, _i32p, _f32p, _int, _int, _int, _stream], _int),
    "usip_index_max_values_f32": ([_f32p, _i32p, _i32p, _i32p, _f32p, _int, _int, _int, _int, _int, _stream], _int),
    "usip_index_max_values_backward_add_f32": ([_f32p, _i32p, _i32p, _f32p, _int, _int, _int, _int, _int, _int,
                                                _stream], _int),
    "usip_index_max_values_backward_f32": ([_f32p, _i32p, _i32p, _i32p, _f32p, _int, _int, _f32p, _int, _int, _int, _int,
                                            _stream], _int),
    "usip_mlp_narrow_forward_blocks": ([_int, _int, _int, _int], _int),
    "usip_mlp_narrow_forward_f32": ([_f32p, _int, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _int, _f32p, _int, _int,
                                     _int, _int, _stream], _int),
    "usip_detector_head_f32": ([_f32p, _f32p, _flt, _f32p, _f32p, _int, _int, _stream], _int),
    "usip_detector_head_backward_f32": ([_f32p, _f32p, _f32p, _f32p, _int, _int, _stream], _int),
    "usip_rigid_transform_f32": ([_f32p, _f32p, _f32p, _f32p, _f32p, _int, _int, _int, _stream], _int),
    "usip_detector_loss_combine_f32": ([_f32p, _f32p, _flt, _f32p, ctypes.c_longlong, _stream], _int),
    "usip_fill_scaled_f32": ([_f32p, _flt, _f32p, ctypes.c_longlong, _stream], _int),
    "usip_mlp_split3_blocks": ([_int, _int, _int], _int),
    "usip_mlp_split3_multi_f32": ([ctypes.c_void_p, _int, _int, _stream], _int),
    "usip_bn_group_dy_sum_f32": ([_f32p, _f32p, _f32p, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_csr_by_index_i32": ([_i32p, _i32p, _i32p, _int, _int, _int, _stream], _int),
    "usip_segment_sum_supported": ([_int, _int], _int),
    "usip_segment_sum_f32": ([_f32p, _i32p, _i32p, _f32p, _int, _int, _int, _int, _int, _int, _stream], _int),
    "usip_nearest_backward_f32": ([_f32p, _f32p, _f32p, _i32p, _f32p, _f32p, _f32p, _int, _int, _int, _int, _stream],
                                  _int),
    "usip_nearest_nd_f32": ([_f32p, _f32p, _f32p, _i32p, _int, _int, _int, _int, _stream], _int),
    "usip_chamfer_prob_f32": ([_f32p, _i32p, _f32p, _i32p, _f32p, _f32p, _f32p, _int, _int, _int, _stream], _int),
    "usip_chamfer_prob_backward_f32": ([_f32p, _f32p, _i32p, _f32p, _i32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p,
                                        _int, _int, _int, _stream], _int),
    "usip_nearest_workspace": ([_int, _int, _int], ctypes.c_longlong),
    "usip_nearest_f32": ([_f32p, _f32p, _f32p, _i32p, _f32p, _i32p, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_tiles": ([_int, _int, _int], _int),
    "usip_mlp_gemm_f32": ([_f32p, _int, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int,
                           _f32p, _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_bf16": ([_f32p, _int, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int,
                            _f32p, _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_f32x3": ([_f32p, _int, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int,
                             _f32p, _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_f32x3_used": ([_int, _int, _int, _int], _int),
    "usip_mlp_x3p_tile_rows": ([_int, _int, _int], _int),
    "usip_mlp_x3p_tile_cols": ([_int, _int, _int, _int, _int], _int),
    "usip_mlp_split3_bytes": ([_int, _int], ctypes.c_longlong),
    "usip_mlp_split3_f32": ([_f32p, _int, _int, _int, _int, ctypes.c_void_p, _stream], _int),
    "usip_mlp_gemm_x3p_f32": ([ctypes.c_void_p, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int,
                               _f32p, _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_x2r_tiles": ([_int, _int], _int),
    "usip_mlp_gemm_x2r_f32": ([ctypes.c_void_p, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int, _f32p,
                               _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_split2h_f32": ([_f32p, _int, _int, _int, _int, ctypes.c_void_p, _stream], _int),
    "usip_mlp_gemm_x2h_f32": ([ctypes.c_void_p, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _i32p, _int,
                               _f32p, _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_x2d_red_tiles": ([_int, _int, _int, _int, _int], _int),
    "usip_mlp_gemm_x2h_red_f32": ([ctypes.c_void_p, _f32p, _f32p, _f32p, _int, _f32p, _i32p, _int, _f32p, _f32p, _f32p, _f32p,
                                   _f32p, _int, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_gemm_x2h_fork_supported": ([_int, _int, _int, _int, _int], _int),
    "usip_mlp_gemm_x2h_fork_f32": ([ctypes.c_void_p, _f32p, _f32p, _f32p, _f32p, _int, _f32p, _i32p, _int, _int, _int, _int,
                                    _int, _stream], _int),
    "usip_mlp_wgrad_f32x3_used": ([_int, _int, _int, _int], _int),
    "usip_bn_pool_backward_reduce_f32": ([_f32p, _i32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _int, _f32p, _f32p,
                                          _f32p, _f32p, _int, _int, _int, _int, _int, _stream], _int),
    "usip_bn_finalize_f32": ([_f32p, _int, _int, ctypes.c_longlong, _f32p, _f32p, _flt, _flt, _f32p, _f32p, _f32p,
                              _f32p, _f32p, _stream], _int),
    "usip_bn_apply_f32": ([_f32p, _f32p, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_bn_backward_reduce_f32": ([_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _f32p, _f32p,
                                     _f32p, _int, _int, _int, _int, _int, _stream], _int),
    "usip_mlp_wgrad_workspace": ([_int, _int, _int, _int], ctypes.c_longlong),
    "usip_mlp_wgrad_f32": ([_f32p, _f32p, _f32p, _int, _f32p, _f32p, _f32p, _i32p, _int, _f32p, _f32p, _int, _int,
                            _int, _int, _int, _int, _stream], _int),
    "usip_mlp_wgrad_bf16": ([_f32p, _f32p, _f32p, _int, _f32p, _f32p, _f32p, _i32p, _int, _f32p, _f32p, _int, _int,
                             _int, _int, _int, _int, _stream], _int),
    "usip_mlp_wgrad_f32x3": ([_f32p, _f32p, _f32p, _int, _f32p, _f32p, _f32p, _i32p, _int, _f32p, _f32p, _int, _int,
                              _int, _int, _int, _int, _stream], _int),
    "usip_mlp_wgrad_x2h_f32": ([_f32p, _f32p, _f32p, _int, _f32p, _f32p, _f32p, _i32p, _int, _f32p, _f32p, _int, _int,
                                _int, _int, _int, _int, _stream], _int),
    "usip_mlp_narrow_backward_supported": ([_int, _int, _int], _int),
    "usip_mlp_narrow_backward_workspace": ([_int, _int, _int], ctypes.c_longlong),
    "usip_mlp_narrow_backward_blocks": ([_int, _int, _int], _int),
    "usip_mlp_layer_backward_x2h_supported": ([_int, _int, _int, _int], _int),
    "usip_mlp_layer_backward_x2h_workspace": ([_int, _int, _int, _int], ctypes.c_longlong),
    "usip_mlp_layer_backward_x2h_blocks": ([_int, _int, _int, _int], _int),
    "usip_mlp_layer_backward_x2h_f32": ([_f32p, _f32p, _f32p, _f32p, _i32p, _int, _f32p, _int, _f32p, ctypes.c_void_p,
                                         _f32p, _int, _f32p, _f32p, _int, _f32p, _f32p, _int, _int, _int, _int, _stream],
                                        _int),
    "usip_mlp_layer_backward_x2h_ws_f32": ([_f32p, _f32p, _f32p, _f32p, _int, _f32p, ctypes.c_void_p, _f32p, _int, _f32p,
                                            _f32p, _int, _f32p, _f32p, _int, _f32p, _f32p, _int, _int, _int, _int, _stream],
                                           _int),
    "usip_mlp_wsum_finalize_f32": ([_f32p, _f32p, _int, _int, _f32p, _f32p, _int, _f32p, _int, _stream], _int),
    "usip_mlp_narrow_backward_f32": ([_f32p, _f32p, _f32p, _f32p, _int, _f32p, _f32p, _int, _f32p, _int, _f32p, _f32p,
                                      _int, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_bn_backward_finalize_f32": ([_f32p, _int, _int, ctypes.c_longlong, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p,
                                       _stream], _int),
    "usip_bn_backward_finalize_max_f32": ([_f32p, _int, _int, ctypes.c_longlong, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p,
                                           _f32p, _int, _f32p, _int, _stream], _int),
    "usip_group_max_act_f32": ([_f32p, _f32p, _int, _f32p, _i32p, _f32p, _int, _int, _int, _int, _stream], _int),
    "usip_group_gather_f32": ([_f32p, _i32p, _f32p, _f32p, _int, _int, _int, _int, _int, _int, _int, _int,
                               _stream], _int),
    "usip_group_gather_backward_f32": ([_f32p, _i32p, _f32p, _int, _int, _int, _int, _int, _int, _int, _stream], _int),
    "usip_group_max_f32": ([_f32p, _f32p, _i32p, ctypes.c_longlong, _int, _stream], _int),
    "usip_group_max_backward_f32": ([_f32p, _i32p, _f32p, ctypes.c_longlong, _int, _stream], _int),
    "usip_group_max_backward_add_f32": ([_f32p, _i32p, _f32p, ctypes.c_longlong, _int, _stream], _int),
    "usip_multi_transpose_f32": ([_f32p, _f32p, _i32p, _int, _int, _stream], _int),
    "usip_adam_step_f32": ([_f32p, _f32p, _f32p, _f32p, _f32p, _flt, _flt, _flt, _flt, ctypes.c_longlong, _stream], _int),
    "usip_adam_step_hyper_f32": ([_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, ctypes.c_longlong, _stream], _int),
    "usip_knn_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _int, _stream], _int),
    "usip_knn_points_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _int, _stream], _int),
    "usip_knn_layer_supported": ([_int, _int, _int], _int),
    "usip_knn_layer_forward_f32": ([_f32p, _f32p, _int, _f32p, _f32p, _i32p, _f32p, _f32p, _int, _int, _int, _int, _int,
                                    _stream], _int),
    "usip_knn_layer_backward_f32": ([_f32p, _f32p, _f32p, _int, _f32p, _i32p, _i32p, _f32p, _f32p, _int, _int, _int, _int,
                                     _int, _stream], _int),
    "usip_fps_f32": ([_f32p, _i32p, _i32p, _int, _int, _int, _stream], _int),
    "usip_nms_f32": ([_f32p, _f32p, _flt, _i32p, _i32p, _int, _int, _stream], _int),
    "usip_ball_query_coords_f32": ([_f32p, _f32p, _i32p, _flt, _int, _int, _int, _int, _stream], _int),
    # f-5 training pairs: the structs go by address (usip_amd/pairs.py builds them)
    "usip_pairs_workspace_bytes": ([ctypes.c_void_p, _int], ctypes.c_longlong),
    "usip_pairs_workspace_offset": ([ctypes.c_void_p, _int, _int], ctypes.c_longlong),
    "usip_pairs_build_f32": ([ctypes.c_void_p, _f32p, ctypes.c_void_p, _int, _i32p, _int, ctypes.c_longlong,
                              ctypes.c_uint64, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                              _stream], _int),
    "usip_pairs_apply_f32": ([ctypes.c_void_p, ctypes.c_void_p, _f32p, ctypes.c_void_p, _int, _i32p, _int,
                              ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, _stream], _int),
    "usip_pairs_build_f32_cpu": ([ctypes.c_void_p, ctypes.c_void_p, _f32p, ctypes.c_void_p, _int, _i32p, _int,
                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p], _int),
    # f-6 evaluation: RANSAC registration, repeatability, counted matching (usip_amd/evaluation.py)
    "usip_ransac_trials_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _dbl, ctypes.c_uint64, ctypes.c_void_p, _i32p,
                                ctypes.c_void_p, _i32p, _stream], _int),
    "usip_ransac_trials_explicit_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _dbl, _i32p, _i32p, ctypes.c_void_p,
                                         _stream], _int),
    "usip_ransac_select_f32": ([_f32p, _f32p, _i32p, _int, _int, _int, _int, _dbl, ctypes.c_uint64, ctypes.c_void_p,
                                _i32p, _i32p] + [ctypes.c_void_p] * 9 + [_stream], _int),
    "usip_compare_transform_f64": ([ctypes.c_void_p] * 2 + [_int] + [ctypes.c_void_p] * 2 + [_stream], _int),
    "usip_repeatability_f32": ([_f32p, _i32p, _f32p, _i32p, ctypes.c_void_p, _dbl, _int, _int, _int, ctypes.c_void_p,
                                _i32p, ctypes.c_void_p, _stream], _int),
    "usip_nearest_nd_counted_f32": ([_f32p, _f32p, _i32p, _i32p, _f32p, _i32p, _int, _int, _int, _int, _stream], _int),
    "usip_ransac_trials_f32_cpu": ([_f32p, _f32p, _i32p, _int, _int, _int, _dbl, ctypes.c_uint64, ctypes.c_void_p, _i32p,
                                    _i32p, ctypes.c_void_p, _i32p, _int], _int),
    "usip_ransac_select_f32_cpu": ([_f32p, _f32p, _i32p, _int, _int, _int, _int, _dbl, ctypes.c_uint64, ctypes.c_void_p,
                                    _i32p, _i32p] + [ctypes.c_void_p] * 9, _int),
    "usip_compare_transform_f64_cpu": ([ctypes.c_void_p] * 2 + [_int] + [ctypes.c_void_p] * 2, _int),
    "usip_repeatability_f32_cpu": ([_f32p, _i32p, _f32p, _i32p, ctypes.c_void_p, _dbl, _int, _int, _int, ctypes.c_void_p,
                                    _i32p, ctypes.c_void_p], _int),
    "usip_nearest_nd_counted_f32_cpu": ([_f32p, _f32p, _i32p, _i32p, _f32p, _i32p, _int, _int, _int, _int], _int),
    # f-7 raw scans prepared: neighbours, normals + curvature, voxel grid average (usip_amd/prepare.py)
    "usip_scan_knn_f32": ([_f32p, _i32p, _int, _int, _i32p, _i32p, _stream], _int),
    "usip_scan_normals_f32": ([_f32p, _i32p, _int, _int, ctypes.c_void_p, ctypes.c_void_p, _f32p, _stream], _int),
    "usip_scan_voxel_keys_f32": ([_f32p, _int, _f32p, _dbl, ctypes.c_void_p, _stream], _int),
    "usip_scan_voxel_average_f32": ([_f32p, ctypes.c_void_p, _i32p, _i32p, _int, _int, _f32p, _stream], _int),
    "usip_scan_knn_f32_cpu": ([_f32p, _int, _int, _i32p, _int], _int),
    "usip_scan_normals_f32_cpu": ([_f32p, _i32p, _int, _int, ctypes.c_void_p, ctypes.c_void_p, _f32p], _int),
    "usip_scan_voxel_keys_f32_cpu": ([_f32p, _int, _f32p, _dbl, ctypes.c_void_p], _int),
    "usip_scan_voxel_average_f32_cpu": ([_f32p, ctypes.c_void_p, _i32p, _i32p, _int, _int, _f32p], _int),
    # f-8 descriptor training batches from posed scans: the structs go by address (usip_amd/desc_pairs.py builds them)
    "usip_desc_pairs_workspace_bytes": ([ctypes.c_void_p, _int], ctypes.c_longlong),
    "usip_desc_pairs_workspace_offset": ([ctypes.c_void_p, _int, _int], ctypes.c_longlong),
    "usip_desc_pairs_build_f32": ([ctypes.c_void_p, ctypes.c_void_p, _i32p, _int, ctypes.c_uint64, ctypes.c_uint64,
                                   ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, _stream], _int),
    "usip_desc_pairs_apply_f32": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _i32p, _int, ctypes.c_void_p,
                                   ctypes.c_void_p, _stream], _int),
    "usip_desc_pairs_build_f32_cpu": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _i32p, _int, ctypes.c_uint64,
                                       ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p], _int),
    # f-9 indoor fragment registration: top-k matching, union, information, overlap (usip_amd/fragments.py); RANSAC is f-6's
    "usip_knn_nd_counted_f32": ([_f32p, _f32p, _i32p, _i32p, _int, _f32p, _i32p, _i32p, _int, _int, _int, _int, _stream],
                                _int),
    "usip_match_union_i32": ([_i32p] * 4 + [_int] * 4 + [_i32p, _i32p, _stream], _int),
    "usip_information_f32": ([_f32p, ctypes.c_void_p, _int, _int, ctypes.c_void_p, _stream], _int),
    "usip_overlap_keys_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, ctypes.c_void_p, _int, _int,
                               ctypes.c_void_p, _stream], _int),
    "usip_overlap_ratio_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, ctypes.c_void_p, _i32p,
                                _i32p, _int, _int, _dbl, _i32p, ctypes.c_void_p, _stream], _int),
    "usip_knn_nd_counted_f32_cpu": ([_f32p, _f32p, _i32p, _i32p, _int, _f32p, _i32p, _i32p, _int, _int, _int, _int, _int],
                                    _int),
    "usip_match_union_i32_cpu": ([_i32p] * 4 + [_int] * 4 + [_i32p, _i32p], _int),
    "usip_information_f32_cpu": ([_f32p, ctypes.c_void_p, _int, _int, ctypes.c_void_p], _int),
    "usip_overlap_keys_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, ctypes.c_void_p, _int, _int,
                                   ctypes.c_void_p], _int),
    "usip_overlap_ratio_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, ctypes.c_void_p,
                                    _i32p, _i32p, _int, _int, _dbl, _int, _i32p, ctypes.c_void_p, _int], _int),
    # f-11 baseline keypoints: ISS saliency and non-maximum suppression (usip_amd/baselines.py)
    "usip_iss_saliency_f32": ([_f32p, _i32p, _i32p, _int, _int, _dbl, _dbl, _dbl, _int, ctypes.c_void_p, _i32p, _i32p,
                               _stream], _int),
    "usip_iss_nms_f32": ([_f32p, _i32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _int, ctypes.c_void_p, _stream], _int),
    "usip_iss_saliency_f32_cpu": ([_f32p, _i32p, _int, _int, _dbl, _dbl, _dbl, _int, ctypes.c_void_p, _i32p, _int], _int),
    "usip_iss_nms_f32_cpu": ([_f32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _int, ctypes.c_void_p, _int], _int),
    # f-12 Fast Global Registration: mutual rows, normalisation, tuple test; the optimisation (usip_amd/fragments.py)
    "usip_fgr_tuples_f32": ([_f32p, _f32p] + [_i32p] * 4 + [_int, _int, ctypes.c_uint64, ctypes.c_void_p, _i32p, _i32p,
                            ctypes.c_void_p, _i32p, _i32p, _i32p, _i32p, _int, _stream], _int),
    "usip_fgr_tuples_explicit_f32": ([_f32p, _f32p] + [_i32p] * 4 + [_int, _int, _i32p, _int, _i32p, _i32p, ctypes.c_void_p,
                                     _i32p, _i32p, _i32p, _stream], _int),
    "usip_fgr_optimize_f32": ([_f32p, _f32p, _i32p, _i32p, ctypes.c_void_p, _i32p, _i32p, _int, _int, _dbl]
                              + [ctypes.c_void_p] * 3 + [_i32p, _stream], _int),
    "usip_fgr_tuples_f32_cpu": ([_f32p, _f32p] + [_i32p] * 4 + [_int, _int, ctypes.c_uint64, ctypes.c_void_p, _i32p, _int,
                                _i32p, _i32p, ctypes.c_void_p, _i32p, _i32p, _i32p, _i32p, _int, _int], _int),
    "usip_fgr_tuples_explicit_f32_cpu": ([_f32p, _f32p] + [_i32p] * 4 + [_int, _int, _i32p, _int, _i32p, _i32p,
                                         ctypes.c_void_p, _i32p, _i32p, _i32p, _int], _int),
    "usip_fgr_optimize_f32_cpu": ([_f32p, _f32p, _i32p, _i32p, ctypes.c_void_p, _i32p, _i32p, _int, _int, _dbl]
                                  + [ctypes.c_void_p] * 3 + [_i32p, _int], _int),
    "usip_fgr_sincos_f64_cpu": ([ctypes.c_void_p, _int, ctypes.c_void_p, ctypes.c_void_p], _int),
    # f-13 trimmed ICP between downsampled fragments: the nearest pass, the whole loop (usip_amd/fragments.py)
    "usip_icp_workspace_bytes": ([_int, _int], ctypes.c_longlong),
    "usip_icp_nearest_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                             + [ctypes.c_void_p] * 2 + [_i32p, _int, _int, _i32p, ctypes.c_void_p, ctypes.c_void_p, _stream],
                             _int),
    "usip_icp_refine_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                            + [ctypes.c_void_p] * 2 + [_i32p, _int, _int, _dbl, _int, _dbl, _dbl, _dbl, ctypes.c_void_p,
                                                       ctypes.c_longlong, ctypes.c_void_p, _i32p, ctypes.c_void_p,
                                                       ctypes.c_void_p, _i32p, ctypes.c_void_p, ctypes.c_void_p, _i32p,
                                                       ctypes.c_void_p, ctypes.c_void_p, _stream], _int),
    "usip_icp_nearest_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                                 + [ctypes.c_void_p] * 2 + [_i32p, _int, _int, _i32p, ctypes.c_void_p, _int], _int),
    "usip_icp_refine_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                                + [ctypes.c_void_p] * 2 + [_i32p, _int, _int, _dbl, _int, _dbl, _dbl, _dbl, ctypes.c_void_p,
                                                           _i32p, ctypes.c_void_p, ctypes.c_void_p, _i32p, ctypes.c_void_p,
                                                           ctypes.c_void_p, _i32p, _i32p, ctypes.c_void_p, _int], _int),
    # f-14 loop closures pruned by pose-graph optimisation: dense information, the optimiser (usip_amd/posegraph.py)
    "usip_icp_information_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                                 + [ctypes.c_void_p] * 2 + [_int, _int, _dbl, ctypes.c_void_p, _i32p, _stream], _int),
    "usip_posegraph_workspace_bytes": ([_int, _int, _int], ctypes.c_longlong),
    "usip_posegraph_optimize_f64": ([_i32p] * 4 + [ctypes.c_void_p] * 3 + [_int, _int, _int, _dbl, _dbl, _int, _int,
                                                                           ctypes.c_void_p, ctypes.c_longlong]
                                    + [ctypes.c_void_p] * 5 + [_i32p, ctypes.c_void_p, _i32p, _stream], _int),
    "usip_icp_information_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p]
                                     + [ctypes.c_void_p] * 2 + [_int, _int, _dbl, ctypes.c_void_p, _i32p, _int], _int),
    "usip_posegraph_optimize_f64_cpu": ([_i32p] * 4 + [ctypes.c_void_p] * 3 + [_int, _int, _int, _dbl, _dbl, _int, _int]
                                        + [ctypes.c_void_p] * 5 + [_i32p, ctypes.c_void_p, _i32p, _int], _int),
    # f-16 baseline keypoints: Harris3D normals and response (usip_amd/baselines.py); the suppression is f-11's
    "usip_harris_normals_f32": ([_f32p, _i32p, _i32p, _int, _int, _dbl, _int, ctypes.c_void_p, _i32p, _stream], _int),
    "usip_harris_response_f32": ([_f32p, _i32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _int, ctypes.c_void_p, _i32p, _i32p,
                                  _stream], _int),
    "usip_harris_normals_f32_cpu": ([_f32p, _i32p, _int, _int, _dbl, _int, ctypes.c_void_p, _i32p, _int], _int),
    "usip_harris_response_f32_cpu": ([_f32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _int, ctypes.c_void_p, _i32p, _int],
                                     _int),
    # f-17 baseline keypoints: SIFT3D voxel average, scale space, 25 nearest and extrema (usip_amd/baselines.py)
    "usip_sift_voxel_keys_f32": ([_f32p, _i32p, _int, _int, _dbl, ctypes.c_void_p, _stream], _int),
    "usip_sift_voxel_average_f32": ([_f32p, _f32p, _int, ctypes.c_void_p, _i32p, _int, _int, _f32p, _f32p, _i32p, _stream],
                                    _int),
    "usip_sift_dog_f32": ([_f32p, _f32p, _i32p, _i32p, _int, _int, _int, ctypes.c_void_p, ctypes.c_void_p, _i32p, _stream],
                          _int),
    "usip_sift_nearest_f32": ([_f32p, _i32p, _i32p, _int, _int, _i32p, _stream], _int),
    "usip_sift_extrema_f32": ([ctypes.c_void_p, _i32p, _i32p, _int, _int, _int, _dbl, ctypes.c_void_p, _i32p, _stream], _int),
    "usip_sift_voxel_keys_f32_cpu": ([_f32p, _i32p, _int, _int, _dbl, ctypes.c_void_p], _int),
    "usip_sift_voxel_average_f32_cpu": ([_f32p, _f32p, _int, ctypes.c_void_p, _int, _int, _f32p, _f32p, _i32p, _int], _int),
    "usip_sift_dog_f32_cpu": ([_f32p, _f32p, _i32p, _int, _int, _int, ctypes.c_void_p, ctypes.c_void_p, _int], _int),
    "usip_sift_exp_f64_cpu": ([ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p], _int),
    "usip_sift_nearest_f32_cpu": ([_f32p, _i32p, _int, _int, _i32p, _int], _int),
    "usip_sift_extrema_f32_cpu": ([ctypes.c_void_p, _i32p, _i32p, _int, _int, _int, _dbl, ctypes.c_void_p, _i32p, _int], _int),
    # f-18 a fragment scene's ground truth: reach at two radii with selection keys, the information sum (usip_amd/ground_truth.py)
    "usip_gt_reach_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p, ctypes.c_void_p, _i32p,
                           ctypes.c_void_p, _int, _int, _dbl, _dbl, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, _i32p,
                           ctypes.c_void_p, ctypes.c_void_p, _stream], _int),
    "usip_gt_information_f32": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, ctypes.c_void_p, _i32p, _i32p,
                                 _int, _int, _int, ctypes.c_void_p, _stream], _int),
    "usip_gt_reach_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, _i32p, _i32p, ctypes.c_void_p,
                               ctypes.c_void_p, _int, _int, _dbl, _dbl, ctypes.c_uint64, ctypes.c_void_p, _int,
                               ctypes.c_void_p, _i32p, ctypes.c_void_p, ctypes.c_void_p, _int], _int),
    "usip_gt_information_f32_cpu": ([_f32p, _int, ctypes.c_void_p, _int, ctypes.c_longlong, _i32p, ctypes.c_void_p, _i32p,
                                     _i32p, _int, _int, _int, ctypes.c_void_p, _int], _int),
    # f-19 baseline descriptor: FPFH's integer SPFH and the weighted gather at keypoints (usip_amd/baselines.py)
    "usip_fpfh_spfh_f32": ([_f32p, _i32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _i32p, _i32p, _i32p, _stream], _int),
    "usip_fpfh_gather_f32": ([_f32p, _i32p, _i32p, _i32p, _i32p, _f32p, _i32p, _int, _int, _int, _dbl, ctypes.c_void_p, _i32p,
                              _stream], _int),
    "usip_fpfh_spfh_f32_cpu": ([_f32p, _i32p, ctypes.c_void_p, _int, _int, _dbl, _i32p, _i32p, _int], _int),
    "usip_fpfh_gather_f32_cpu": ([_f32p, _i32p, _i32p, _i32p, _f32p, _i32p, _int, _int, _int, _dbl, ctypes.c_void_p, _i32p,
                                  _int], _int),
}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "usip_amd: %s is missing. Build it with `python -m usip_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback." % LIB_PATH)
        # PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's).  The tensors we
        # are handed live in THAT runtime, so it must be the one already loaded when our library's
        # dependency is resolved: import torch first, then check that exactly one HIP runtime is mapped.
        import torch  # noqa: F401
        try:
            l = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise RuntimeError("usip_amd: cannot load %s: %s" % (LIB_PATH, e)) from e
        try:
            with open("/proc/self/maps") as f:
                runtimes = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
        except OSError:
            runtimes = []
        if len(runtimes) > 1:
            raise RuntimeError("usip_amd: two HIP runtimes are loaded (%s); import torch before anything "
                               "that links libamdhip64" % ", ".join(runtimes))
        for name, (args, res) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        # ctypes cannot see a changed signature, and results depend on three compile flags (an SLP-vectorised build gave
        # rare wrong values on gfx950): the library says what it is, anything else is refused
        ver = l.usip_version().decode()
        if ("abi=%d" % ABI) not in ver.split() or "flags=no-contract,no-fast-math,no-slp" not in ver.split():
            raise RuntimeError("usip_amd: %s reports %r; this package needs abi=%d built by usip_amd/build.py "
                               "(-ffp-contract=off -fno-fast-math -fno-slp-vectorize)" % (LIB_PATH, ver, ABI))
        # measurement knobs for same-box A/B runs: USIP_TUNE="x3_gemm_tile=3,index_max_ch=4" (include/usip_hip.h)
        for item in filter(None, os.environ.get("USIP_TUNE", "").split(",")):
            name, _, value = item.partition("=")
            if l.usip_set_tuning(name.strip().encode(), int(value)) != 0:
                raise RuntimeError("usip_amd: USIP_TUNE names an unknown knob or value: %r" % item)
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError("usip_amd: %s: invalid argument (USIP_EINVAL)" % what)
    raise RuntimeError("usip_amd: %s: HIP error %d" % (what, rc))
