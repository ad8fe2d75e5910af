"""ctypes binding of libctd_hip.so: the C ABI of the headers under include/, one table of TABLES per header.

There is no fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libctd_hip.so")

_c_int, _c_long, _c_float, _c_size_t, _vp = (ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t,
                                             ctypes.c_void_p)
_c_i64 = ctypes.c_int64

class PatternLevel(ctypes.Structure):
    """ctd_pattern_level of include/ctd_hip.h"""
    _fields_ = [("disp", _vp), ("im", _vp), ("mask", _vp), ("pattern", _vp), ("pattern_proj", _vp), ("grad_proj", _vp),
                ("grad_disp", _vp), ("B", _c_int), ("H", _c_int), ("W", _c_int)]


_levels_p = ctypes.POINTER(PatternLevel)


class HdTables(ctypes.Structure):
    """ctd_hd_tables of include/ctd_hip.h (the packed HyperDepth forests of a row range)"""
    _fields_ = [("nodes", _vp), ("roots", _vp), ("leaf_off", _vp), ("leaf_sum", _vp), ("entries", _vp),
                ("n_nodes", ctypes.c_int64), ("n_leaves", ctypes.c_int64), ("n_entries", ctypes.c_int64),
                ("row0", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_trees", ctypes.c_int32),
                ("n_classes", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("reserved", ctypes.c_int32)]

class HdTrainParams(ctypes.Structure):
    """ctd_hd_train_params of include/ctd_hip.h"""
    _fields_ = [(k, ctypes.c_int32) for k in ("n_trees", "max_tree_depth", "n_test_split_functions",
                                              "n_test_thresholds", "n_test_samples", "min_samples_to_split",
                                              "min_samples_for_leaf", "depth_switch", "n_disp_bins", "reserved")] + \
        [("seed", ctypes.c_uint64)]


class HdTrainOut(ctypes.Structure):
    """ctd_hd_train_out of include/ctd_hip.h (device output buffers of a training call and their capacities)"""
    _fields_ = [("nodes", _vp), ("roots", _vp), ("leaf_off", _vp), ("leaf_sum", _vp), ("entries", _vp), ("used", _vp),
                ("cap_nodes", ctypes.c_int64), ("cap_leaves", ctypes.c_int64), ("cap_entries", ctypes.c_int64)]

# header under include/ -> {name: (restype, argtypes)}, one entry per prototype of that header and in the order in which
# the headers were added; lib() binds every table, tests/test_abi_and_host.py holds each against its header
TABLES = {}

# mirrors include/ctd_hip.h one to one.  SIGNATURES stays as the name of this one table, the drop-in interface: the host
# answers recorded in tests/abi_rejections.py and the per-op host tests look its entry points up under that name
SIGNATURES = TABLES["ctd_hip.h"] = {
    "ctd_version": (_c_int, []),
    "ctd_status_string": (ctypes.c_char_p, [_c_int]),
    "ctd_xcorrvol_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_xcorrvol_f32": (_c_int, [_vp, _vp, _c_long, _vp] + [_c_int] * 7 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_xcorrvol_pattern_prepare_f32": (_c_int, [_vp, _c_long] + [_c_int] * 6 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_xcorrvol_f64": (_c_int, [_vp, _vp, _c_long, _vp] + [_c_int] * 6 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_argmax_disp_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_c_int, _vp]),
    "ctd_xcorrvol_rank_supported": (_c_int, [_c_int] * 5),
    "ctd_xcorrvol_rank_layout": (_c_int, [_c_int] * 5 + [ctypes.POINTER(_c_size_t)]),
    "ctd_xcorrvol_argmax_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_xcorrvol_argmax_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 7 + [_c_float, _vp, _c_size_t,
                                                                                          _c_int, _vp]),
    "ctd_lcn_xcorrvol_supported": (_c_int, [_c_int] * 5),
    "ctd_lcn_xcorrvol_argmax_f32": (_c_int, [_vp, _vp, _vp, _c_int, _c_float, _c_int, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 6 +
                                    [_c_float, _vp, _c_size_t, _c_int, _vp]),
    "ctd_photometric_fwd_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_photometric_fwd_f64": (_c_int, [_vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_photometric_bwd_f32": (_c_int, [_vp, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_photometric_bwd_f64": (_c_int, [_vp, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_photometric_fwd_fast_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_photometric_bwd_fast_f32": (_c_int, [_vp, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_costvol_f32": (_c_int, [_vp, _vp, _c_long, _vp] + [_c_int] * 6 + [_c_float, _c_int, _vp]),
    "ctd_costvol_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_costvol_fast_f32": (_c_int, [_vp, _vp, _c_long, _vp] + [_c_int] * 6 + [_c_float, _vp, _c_size_t, _c_int, _vp]),
    "ctd_costvol_argmin_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_costvol_argmin_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_float, _vp, _c_size_t,
                                                                                     _c_int, _vp]),
    "ctd_xcorrvol_subpixel_workspace_bytes": (_c_size_t, [_c_int] * 6),
    "ctd_xcorrvol_subpixel_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 6 + [_vp, _c_size_t, _c_int,
                                                                                          _vp]),
    "ctd_costvol_subpixel_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _c_int,
                                                                                         _vp]),
    "ctd_match_validity_f32": (_c_int, [_vp, _c_int, _vp, _vp, _vp, _vp] + [_c_int] * 5 + [_c_float, _c_int, _vp]),
    "ctd_xcorrvol_validity_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_xcorrvol_validity_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _vp] + [_c_int] * 8 + [_c_float, _vp, _c_size_t,
                                                                                               _c_int, _vp]),
    "ctd_costvol_validity_workspace_bytes": (_c_size_t, [_c_int] * 8),
    "ctd_costvol_validity_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int, _c_int,
                                                                                              _c_float, _vp, _c_size_t,
                                                                                              _c_int, _vp]),
    "ctd_sgm_workspace_bytes": (_c_size_t, [_c_int] * 6),
    "ctd_sgm_aggregate_f32": (_c_int, [_vp, _c_int, _c_float, _c_float, _c_int, _vp, _vp, _vp] + [_c_int] * 4 +
                              [_vp, _c_size_t, _c_int, _vp]),
    "ctd_disp_components_workspace_bytes": (_c_size_t, [_c_int] * 3),
    "ctd_disp_components_f32": (_c_int, [_vp, _vp, _c_float, _c_int, _vp, _vp] + [_c_int] * 3 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_disp_speckle_f32": (_c_int, [_vp, _vp, _c_float, _c_int, _c_int, _vp, _vp] + [_c_int] * 3 +
                             [_vp, _c_size_t, _c_int, _vp]),
    "ctd_disp_median_f32": (_c_int, [_vp, _vp, _c_int, _c_int, _vp, _vp] + [_c_int] * 4 + [_vp]),
    "ctd_depth_consistency_f32": (_c_int, [_vp] * 6 + [_c_float, _c_float, _c_int] + [_vp] * 3 + [_c_int] * 4 + [_c_int, _vp]),
    "ctd_depth_fuse_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "ctd_depth_fuse_points_f32": (_c_int, [_vp] * 6 + [_c_float, _c_float, _c_int, _c_int] + [_vp] * 6 + [_c_int] * 4 +
                                  [_vp, _c_size_t, _c_int, _vp]),
    "ctd_lcn_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_c_float, _c_int, _vp]),
    "ctd_lcn_fast_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_c_float, _c_int, _vp]),
    "ctd_lcn_datagen_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_c_float, _c_int, _vp]),
    "ctd_disp_to_depth_fwd_f32": (_c_int, [_vp, _vp, _c_long, _c_float, _c_int, _vp]),
    "ctd_idx_to_depth_f32": (_c_int, [_vp, _vp, _c_long, _c_float, _c_float, _c_int, _vp]),
    "ctd_disp_to_depth_bwd_f32": (_c_int, [_vp, _vp, _vp, _c_long, _c_float, _c_int, _vp]),
    "ctd_disparity_loss_workspace_bytes": (_c_size_t, [_c_int] * 3),
    "ctd_disparity_loss_fwd_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 3 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_disparity_loss_bwd_f32": (_c_int, [_vp] * 5 + [_c_int] * 3 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_geometric_workspace_bytes": (_c_size_t, [_c_int] * 3),
    "ctd_geometric_fwd_f32": (_c_int, [_vp] * 9 + [_c_int] * 4 + [_c_float, _vp, _c_size_t, _c_int, _vp]),
    "ctd_geometric_sym_fwd_f32": (_c_int, [_vp] * 9 + [_c_int] * 3 + [_c_float, _vp, _c_size_t, _vp, _c_int, _vp]),
    "ctd_geometric_bwd_f32": (_c_int, [_vp] * 10 + [_c_int, _vp] + [_c_int] * 3 + [_c_float, _c_int, _vp]),
    "ctd_pattern_loss_workspace_bytes": (_c_size_t, [_c_int] * 3),
    "ctd_pattern_loss_fwd_f32": (_c_int, [_vp] * 6 + [_c_int] * 4 + [_c_float, _vp, _c_size_t, _c_int, _vp]),
    "ctd_pattern_loss_bwd_f32": (_c_int, [_vp] * 8 + [_c_int] * 4 + [_c_float, _c_int, _vp]),
    "ctd_pattern_loss_multi_workspace_bytes": (_c_size_t, [_c_int, _levels_p]),
    "ctd_pattern_loss_multi_fwd_f32": (_c_int, [_c_int, _levels_p, _vp, _c_int, _c_float, _vp, _c_size_t, _c_int, _vp]),
    "ctd_pattern_loss_multi_bwd_f32": (_c_int, [_c_int, _levels_p, _vp, _vp, _c_int, _c_float, _c_int, _vp]),
    "ctd_render_mesh_proj_f32": (_c_int, [_vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp,
                                          _c_float, _c_float, _vp, _vp, _vp, _c_int, _vp]),
    "ctd_render_mesh_f32": (_c_int, [_vp, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp]),
    "ctd_mesh_bvh_bytes": (_c_size_t, [_c_int]),
    "ctd_mesh_bvh_workspace_bytes": (_c_size_t, [_c_int]),
    "ctd_mesh_bvh_build_f32": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_size_t, _vp, _c_size_t, _vp, _c_int, _vp]),
    "ctd_render_mesh_proj_bvh_f32": (_c_int, [_vp, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                              _vp, _vp, _c_float, _c_float, _vp, _vp, _vp, _c_int, _vp]),
    "ctd_render_mesh_bvh_f32": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp,
                                         _c_int, _vp]),
    "ctd_syn_finish_f32": (_c_int, [_vp] * 4 + [ctypes.c_double, _c_float, _c_int, _c_float, _c_int] + [_vp] * 5 +
                           [_c_int] * 3 + [_c_int, _vp]),
    "ctd_augment_f32": (_c_int, [_vp, _vp, _c_int, _vp, _vp, _vp] + [_c_int] * 3 + [_c_int, _vp]),
    "ctd_salt_pepper_f32": (_c_int, [_vp] * 5 + [_c_int] * 4 + [_c_int, _vp]),
    "ctd_nn_f32": (_c_int, [_vp, _vp, _c_long, _c_long, _vp, _c_int, _vp]),
    "ctd_nn_f64": (_c_int, [_vp, _vp, _c_long, _c_long, _vp, _c_int, _vp]),
    "ctd_crosscheck": (_c_int, [_vp, _vp, _c_long, _c_long, _vp, _c_int, _vp]),
    "ctd_proj_nn_f32": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_vp, _c_int, _vp]),
    "ctd_proj_nn_f64": (_c_int, [_vp, _vp, _vp] + [_c_int] * 4 + [_vp, _c_int, _vp]),
    "ctd_hyperdepth_eval_f32": (_c_int, [ctypes.POINTER(HdTables), _vp] + [_c_int] * 6 + [_vp, _c_int, _vp]),
    "ctd_hyperdepth_train_count_f32": (_c_int, [_vp] + [_c_int] * 6 + [_vp, _c_int, _vp]),
    "ctd_hyperdepth_train_workspace_bytes": (_c_size_t, [ctypes.POINTER(HdTrainParams), _c_int, _vp, ctypes.c_int64]),
    "ctd_hyperdepth_train_f32": (_c_int, [ctypes.POINTER(HdTrainParams), _vp, _c_int, _vp, _vp] + [_c_int] * 5 +
                                 [_vp, _vp, _c_size_t, ctypes.POINTER(HdTrainOut), _c_int, _vp]),
}

# measurement hooks of include/ctd_hip_bench.h (bench.py, tools/): not part of the drop-in interface
TABLES["ctd_hip_bench.h"] = {
    "ctd_kernel_timing_enable": (None, [_c_int]),
    "ctd_kernel_timing_collect": (_c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_int)]),
}

# band-limited matching of include/ctd_hip_band.h (an addition beside ctd_hip.h; torchext.xcorrvol_argmax_band, ...)
TABLES["ctd_hip_band.h"] = {
    "ctd_xcorrvol_argmax_band_workspace_bytes": (_c_size_t, [_c_int] * 6),
    "ctd_xcorrvol_argmax_band_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _vp] + [_c_int] * 6 + [_vp, _c_size_t,
                                                                                                  _c_int, _vp]),
    "ctd_costvol_argmin_band_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _vp] + [_c_int] * 6 + [_c_float, _c_int,
                                                                                                 _vp]),
}

# forward depth warping and the windowed band of include/ctd_hip_warp.h (an addition beside ctd_hip.h and ctd_hip_band.h;
# torchext.depth_warp, torchext.disparity_band_window)
TABLES["ctd_hip_warp.h"] = {
    "ctd_depth_warp_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "ctd_depth_warp_f32": (_c_int, [_vp] * 8 + [_c_int, _vp, _vp] + [_c_int] * 4 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_disparity_band_window_f32": (_c_int, [_vp, _c_float, _c_int, _c_int, _c_int, _vp, _vp] + [_c_int] * 3 +
                                      [_c_int, _vp]),
}

# match validity of the band matchers of include/ctd_hip_band_validity.h (an addition beside the headers above;
# torchext.xcorrvol_band_validity, torchext.costvol_band_validity)
TABLES["ctd_hip_band_validity.h"] = {
    "ctd_xcorrvol_band_validity_f32": (_c_int, [_vp, _vp, _c_long] + [_vp] * 7 + [_c_int] * 6 + [_c_float, _c_int, _vp,
                                                                                             _c_size_t, _c_int, _vp]),
    "ctd_costvol_band_validity_f32": (_c_int, [_vp, _vp, _c_long] + [_vp] * 7 + [_c_int] * 6 + [_c_float, _c_int,
                                                                                            _c_float, _c_int, _vp]),
}

# depth-map normals and point-to-plane ICP of include/ctd_hip_icp.h (an addition beside the headers above;
# torchext.depth_normals, torchext.depth_icp_system, torchext.depth_icp_update, torchext.depth_icp)
TABLES["ctd_hip_icp.h"] = {
    "ctd_depth_normals_f32": (_c_int, [_vp] * 3 + [_c_float, _vp] + [_c_int] * 4 + [_c_int, _vp]),
    "ctd_depth_icp_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "ctd_depth_icp_system_f32": (_c_int, [_vp] * 8 + [_c_float] + [_vp] * 3 + [_c_int] * 4 + [_vp, _c_size_t, _c_int, _vp]),
    "ctd_depth_icp_update_f32": (_c_int, [_vp] * 4 + [_c_int, ctypes.c_double, ctypes.c_double] + [_vp] * 3 +
                                 [_c_int] * 2 + [_c_int, _vp]),
}

# truncated signed distance volumes of include/ctd_hip_tsdf.h (an addition beside the headers above;
# torchext.tsdf_volume, torchext.tsdf_integrate, torchext.tsdf_surface_points, torchext.tsdf_raycast)
TABLES["ctd_hip_tsdf.h"] = {
    "ctd_tsdf_integrate_f32": (_c_int, [_vp] * 3 + [_c_float] + [_vp] * 6 + [_c_float, _c_float] + [_c_int] * 7 + [_c_int, _vp]),
    "ctd_tsdf_surface_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "ctd_tsdf_surface_points_f32": (_c_int, [_vp] * 3 + [_c_float, _c_float] + [_vp] * 4 + [ctypes.c_int64] + [_c_int] * 4 +
                                    [_vp, _c_size_t, _c_int, _vp]),
    "ctd_tsdf_raycast_f32": (_c_int, [_vp] * 3 + [_c_float] + [_vp] * 3 + [_c_float, _c_float, _c_int, _c_float, _vp] +
                             [_c_int] * 7 + [_c_int, _vp]),
}

# marching cubes over a volume of include/ctd_hip_mesh.h (an addition beside the headers above; mesh.tsdf_mesh)
TABLES["ctd_hip_mesh.h"] = {
    "ctd_tsdf_mesh_workspace_bytes": (_c_size_t, [_c_int] * 4),
    "ctd_tsdf_mesh_faces_i32": (_c_int, [_vp, _vp, _c_float, _vp, _vp, ctypes.c_int64] + [_c_int] * 4 + [_vp, _c_size_t, _c_int,
                                                                                                    _vp]),
    "ctd_tsdf_mesh_case": (_c_int, [_c_int, ctypes.POINTER(ctypes.c_int32)]),
}

# mesh clean-up of include/ctd_hip_mesh_clean.h (an addition beside the headers above; meshops.mesh_components,
# meshops.mesh_clean, meshops.clean_tsdf_mesh)
TABLES["ctd_hip_mesh_clean.h"] = {
    "ctd_mesh_clean_workspace_bytes": (_c_size_t, [_c_i64, _c_i64]),
    "ctd_mesh_components_i32": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _vp, _vp, _vp, _vp, _c_size_t, _c_int, _vp]),
    "ctd_mesh_clean_i32": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _c_int, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp,
                                    _c_size_t, _c_int, _vp]),
}

# nearest-face queries of include/ctd_hip_mesh_dist.h (an addition beside the headers above; mesheval.point_mesh_distance,
# mesheval.reconstruction_error)
TABLES["ctd_hip_mesh_dist.h"] = {
    "ctd_point_mesh_distance_f32": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp, _c_int, _vp]),
}

# colours for mesh points from a track's views of include/ctd_hip_mesh_color.h (an addition beside the headers above;
# meshcolor.view_colors, meshcolor.color_tsdf_mesh)
TABLES["ctd_hip_mesh_color.h"] = {
    "ctd_mesh_view_colors_f32": (_c_int, [_vp, _vp, _c_int] + [_vp] * 5 + [_c_int] * 4 + [_vp, _c_int, _vp, _c_int, _vp,
                                                                                       _c_float, _c_float, _c_int] +
                                 [_vp] * 4 + [_c_int, _vp]),
}

# connectivity by vertex, Taubin smoothing and vertex normals of include/ctd_hip_mesh_smooth.h (an addition beside the
# headers above; meshsmooth.MeshAdjacency, meshsmooth.mesh_smooth, meshsmooth.vertex_normals, meshsmooth.smooth_tsdf_mesh)
TABLES["ctd_hip_mesh_smooth.h"] = {
    "ctd_mesh_adjacency_workspace_bytes": (_c_size_t, [_c_i64, _c_i64]),
    "ctd_mesh_adjacency_i32": (_c_int, [_vp, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_size_t, _c_int,
                                        _vp]),
    "ctd_mesh_smooth_workspace_bytes": (_c_size_t, [_c_i64]),
    "ctd_mesh_smooth_f32": (_c_int, [_vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_float, _c_float, _c_int, _vp, _vp, _c_size_t,
                                     _c_int, _vp]),
    "ctd_mesh_vertex_normals_f32": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _vp]),
}

# vertex clustering with quadric placement of include/ctd_hip_mesh_simplify.h (an addition beside the headers above;
# meshsimplify.mesh_simplify, meshsimplify.simplify_tsdf_mesh)
TABLES["ctd_hip_mesh_simplify.h"] = {
    "ctd_mesh_simplify_workspace_bytes": (_c_size_t, [_c_i64, _c_i64]),
    "ctd_mesh_simplify_f32": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _c_float, _c_float, _c_float, _c_float,
                                       ctypes.c_double, _c_int, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_size_t, _c_int,
                                       _vp]),
}

# signed nearest-face queries of include/ctd_hip_mesh_sdf.h (an addition beside the headers above;
# meshsdf.point_mesh_signed_distance, meshsdf.mesh_to_tsdf, meshsdf.signed_error)
TABLES["ctd_hip_mesh_sdf.h"] = {
    "ctd_point_mesh_signed_f32": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp, _c_i64, _vp, _c_float, _vp, _vp, _vp,
                                           _vp, _vp, _c_int, _vp]),
}

_lib = None


def lib():
    """Loads the HIP library; raises if it has not been built (python -m connecting_the_dots_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "connecting_the_dots_amd: %s is missing -- build it with "
                "`python -m connecting_the_dots_amd.build` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for table in TABLES.values():
            for name, (res, args) in table.items():
                fn = getattr(l, name)       # AttributeError here means header / library mismatch
                fn.restype = res
                fn.argtypes = args
        _lib = l
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().ctd_status_string(status).decode()
        raise RuntimeError("%s failed: %s (status %d)" % (what, msg, status))
