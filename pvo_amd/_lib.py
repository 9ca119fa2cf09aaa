"""ctypes binding of libpvo_hip.so (the C ABI declared in include/pvo_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is
missing, or a call returns a non-zero status, this raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpvo_hip.so")

PVO_F32, PVO_F16, PVO_BF16, PVO_F64 = 0, 1, 2, 3
PVO_ABI_VERSION = 106          # include/pvo_hip.h

_c = ctypes
_vp, _i, _f, _sz = _c.c_void_p, _c.c_int, _c.c_float, _c.c_size_t

# name -> (restype, argtypes); mirrors include/pvo_hip.h one to one
SIGNATURES = {
    "pvo_strerror": (_c.c_char_p, [_i]),
    "pvo_version": (_i, []),
    "pvo_graph_update_args_size": (_sz, []),
    "pvo_last_hip_error": (_c.c_char_p, []),
    "pvo_debug_config": (_i, [_i, _i]),
    "pvo_knob": (_i, [_i]),
    "pvo_debug_trunk_range": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pvo_corr_index_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_corr_index_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_corr_pyramid_lookup": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pvo_altcorr_forward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_altcorr_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_corr_build": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pvo_gru_glo_chunks": (_i, [_i]),
    "pvo_gru_glo_fused": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pvo_gate_context": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "pvo_gru_conv_gates": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_gru_conv_candidate": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_conv3x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_conv3x3_c128": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_conv7x7_c8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_flow_encoder": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_corr_encode": (_i, [_vp, _vp, _vp, _vp, _c.c_longlong, _i, _vp]),
    "pvo_eta_head": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp]),
    "pvo_conv1x1_c128": (_i, [_vp, _vp, _vp, _vp, _c.c_longlong, _i, _i, _i, _vp]),
    "pvo_corr_build_tiled": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pvo_corr_build_tiled_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pvo_corr_lookup_encode_tiled": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "pvo_corr_pyramid_lookup_tiled": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pvo_heads_out": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_conv3x3_heads": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_heads_gather": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_segment_mean": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_graph_motion": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_reproject_motion": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_bias_norm_act": (_i, [_vp, _vp, _vp, _vp, _c.c_longlong, _i, _i, _i, _f, _i, _i, _i, _vp]),
    "pvo_bias_norm_act_slices": (_i, [_i]),
    "pvo_bias_norm_act_split": (_i, [_vp, _vp, _vp, _vp, _c.c_longlong, _i, _i, _i, _f, _i, _i, _i, _vp, _sz, _vp]),
    "pvo_conv1x1_planes": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_conv_planes_supported": (_i, [_i, _i, _i, _i]),
    "pvo_conv_planes_filter_bytes": (_sz, [_i, _i, _i]),
    "pvo_conv_planes_pack": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_conv_planes": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_cvx_upsample": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pvo_cvx_upsample_vjp_scratch_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "pvo_cvx_upsample_vjp": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "pvo_frame_normalise": (_i, [_vp, _vp, _i, _i, _c.POINTER(_f), _c.POINTER(_f), _i, _i, _vp]),
    "pvo_segment_hist": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "pvo_graph_post": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _i, _f, _i, _vp]),
    "pvo_operator_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pvo_update_operator": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_graph_update_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "pvo_graph_update": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_graph_update_rig": (_i, [_vp, _vp, _vp, _sz, _f, _vp]),
    "pvo_update_operator_rows": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "pvo_graph_update_rows": (_i, [_vp, _vp, _vp, _sz, _f, _vp, _vp]),
    "pvo_edge_rows_init": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pvo_se3_unary": (_i, [_i, _vp, _vp, _c.c_longlong, _i, _vp]),
    "pvo_se3_binary": (_i, [_i, _vp, _c.c_longlong, _vp, _c.c_longlong, _vp, _c.c_longlong, _i, _vp]),
    "pvo_se3_unary_vjp": (_i, [_i, _vp, _vp, _vp, _c.c_longlong, _i, _vp]),
    "pvo_se3_binary_vjp": (_i, [_i, _vp, _c.c_longlong, _vp, _c.c_longlong, _vp, _vp, _vp, _c.c_longlong, _i, _vp]),
    "pvo_proj_transform": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pvo_proj_transform_vjp": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pvo_side_stream": (_i, [_c.POINTER(_vp)]),
    "pvo_proximity_select": (_i, [_vp, _i, _i, _i, _i, _i, _i, _c.c_double, _vp, _vp, _i, _vp, _vp, _i, _c.POINTER(_i)]),
    "pvo_probe_arm": (_i, [_i, _i]),
    "pvo_probe_arm_every": (_i, [_i, _i, _i]),
    "pvo_probe_read": (_i, [_vp, _i]),
    "pvo_frame_distance": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pvo_frame_distance_bidirectional": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pvo_projmap": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pvo_iproj": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pvo_depth_filter": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pvo_reproject": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pvo_ba_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pvo_ba": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i,
                    _f, _f, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "pvo_ba_plan": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "pvo_ba_depth_prior": (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _f, _vp]),
    "pvo_ba_prior": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i,
                          _f, _f, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp, _f, _vp]),
    "pvo_depth_sense": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "pvo_ba_stereo": (_i, [_vp, _sz, _i, _i, _i, _i, _f, _vp]),
    "pvo_ba_rig": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i,
                        _f, _f, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp, _f, _f, _vp]),
    "pvo_ba_sigma": (_i, [_vp, _vp, _sz, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "pvo_ba_uncertainty": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f,
                                _vp, _vp, _vp, _vp, _vp, _sz, _vp, _f, _f, _vp]),
    "pvo_ba_calib_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pvo_ba_calib": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _i,
                          _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "pvo_reproject_rig": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pvo_reproject_motion_rig": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "pvo_map_points_args_size": (_sz, []),
    "pvo_map_points_workspace_bytes": (_sz, [_i, _i, _i]),
    "pvo_map_points": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_integrate_args_size": (_sz, []),
    "pvo_tsdf_integrate_workspace_bytes": (_sz, [_i]),
    "pvo_tsdf_integrate": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_mesh_args_size": (_sz, []),
    "pvo_tsdf_mesh_workspace_bytes": (_sz, [_i, _i, _i]),
    "pvo_tsdf_mesh": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_allocate_args_size": (_sz, []),
    "pvo_tsdf_sparse_allocate_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pvo_tsdf_sparse_allocate": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_integrate_args_size": (_sz, []),
    "pvo_tsdf_sparse_integrate_workspace_bytes": (_sz, [_i]),
    "pvo_tsdf_sparse_integrate": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_mesh_args_size": (_sz, []),
    "pvo_tsdf_sparse_mesh_workspace_bytes": (_sz, [_i]),
    "pvo_tsdf_sparse_mesh": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_panoptic_args_size": (_sz, []),
    "pvo_tsdf_mesh_labels_args_size": (_sz, []),
    "pvo_tsdf_integrate_panoptic": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_integrate_panoptic": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_tsdf_mesh_panoptic": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_mesh_panoptic": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pvo_tsdf_render_args_size": (_sz, []),
    "pvo_tsdf_render_workspace_bytes": (_sz, [_i]),
    "pvo_tsdf_render": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_render_args_size": (_sz, []),
    "pvo_tsdf_sparse_render_workspace_bytes": (_sz, [_i]),
    "pvo_tsdf_sparse_render": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_track_args_size": (_sz, []),
    "pvo_tsdf_track_workspace_bytes": (_sz, [_i, _i, _i]),
    "pvo_tsdf_track": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_track_args_size": (_sz, []),
    "pvo_tsdf_sparse_track_workspace_bytes": (_sz, [_i, _i, _i]),
    "pvo_tsdf_sparse_track": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_reintegrate_args_size": (_sz, []),
    "pvo_tsdf_reintegrate_workspace_bytes": (_sz, [_i, _i]),
    "pvo_tsdf_reintegrate": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_tsdf_sparse_reintegrate_args_size": (_sz, []),
    "pvo_tsdf_sparse_reintegrate_workspace_bytes": (_sz, [_i, _i]),
    "pvo_tsdf_sparse_reintegrate": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_object_motion_args_size": (_sz, []),
    "pvo_object_motion_workspace_bytes": (_sz, [_i, _i, _i]),
    "pvo_object_motion": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_segment_assoc_args_size": (_sz, []),
    "pvo_segment_associate": (_i, [_vp, _vp]),
    "pvo_feature_transport_args_size": (_sz, []),
    "pvo_feature_transport_workspace_bytes": (_sz, [_vp]),
    "pvo_feature_transport": (_i, [_vp, _vp, _sz, _vp]),
    "pvo_ba_last_partition": (_i, [_vp, _sz, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), _vp]),
    "pvo_ba_packed_elems": (_sz, [ctypes.POINTER(ctypes.c_int), _i]),
    "pvo_ba_pack": (_i, [_vp, _vp, _vp, _i, _vp]),
    "pvo_ba_finish_packed": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _i, _f,
                                  _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "pvo_ba_local": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i,
                          _i, _vp, _vp, _sz, _vp]),
    "pvo_ba_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _i, _f,
                           _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "pvo_ba_finish_graph": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _i, _f,
                                 _vp, _vp, _i, _vp, _vp, _sz, _i, _vp]),
    "pvo_ba_solve_kind": (_i, [_i, _i, _i]),
    "pvo_ba_finish_riders": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _i, _f,
                                  _vp, _vp, _i, _vp, _vp, _sz, _vp, _vp]),
    "pvo_ba_finish_conv1x1": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _i, _f,
                                   _vp, _vp, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _c.c_longlong, _i, _i, _vp]),
    "pvo_ba_train_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "pvo_ba_train_vjp_scratch_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "pvo_ba_train": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i,
                          _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    "pvo_ba_train_vjp": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i,
                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _i, _vp]),
}



class UpdateWeights(_c.Structure):
    """pvo_update_weights (include/pvo_hip.h)"""
    _fields_ = [("dtype", _i), ("flags", _i)] + [(n, _vp) for n in (
        "enc0_w", "enc0_b", "cenc2_w", "cenc2_b", "fenc0_w", "fenc0_b", "fenc2_w", "fenc2_b", "glo_w", "glo_b",
        "gate_wt", "gate_b", "zr_w", "q_w", "zr_inp_w", "q_inp_w", "heads1_w", "heads1_b", "heads2_w", "heads2_b",
        "agg1_w", "agg1_b", "agg2_w", "agg2_b", "eta_w", "eta_b", "up_w", "up_b")]


class OperatorArgs(_c.Structure):
    """pvo_operator_args"""
    _fields_ = [("E", _i), ("H", _i), ("W", _i), ("levels", _vp * 4), ("slots", _vp), ("num_slots", _i),
                ("coords", _vp), ("corr", _vp), ("motion", _vp), ("net", _vp), ("net_out", _vp), ("inp", _vp),
                ("P_zr", _vp), ("P_q", _vp), ("static_by_slot", _i), ("seg_ptr", _vp), ("seg_idx", _vp), ("K", _i), ("heads", _vp),
                ("eta_frame", _vp), ("eta_pos", _vp), ("R", _i), ("damping", _vp), ("EP", _f), ("eta_scale", _f), ("eta", _vp),
                ("upmask", _vp)]


class GraphUpdateArgs(_c.Structure):
    """pvo_graph_update_args"""
    _fields_ = [("op", OperatorArgs), ("nframes", _i), ("poses", _vp), ("disps", _vp), ("intrinsics", _vp),
                ("ii", _vp), ("jj", _vp), ("target", _vp), ("delta_dy", _vp), ("raw_mask", _vp), ("weight", _vp),
                ("full_flow", _vp), ("segm", _vp), ("max_segments", _i), ("vote_thresh", _f), ("dy_thresh", _f),
                ("n_in", _i), ("target_ba", _vp), ("weight_ba", _vp), ("ii_ba", _vp), ("jj_ba", _vp),
                ("t0", _i), ("t1", _i), ("itrs", _i), ("motion_only", _i), ("lm", _f), ("ep", _f),
                ("sys", _vp), ("ba_ws", _vp), ("ba_ws_bytes", _sz), ("clamp_frames", _i), ("disp_min", _f),
                ("want_upmask", _i), ("context_ahead", _i), ("context_ready", _i),
                ("want_upsample", _i), ("disps_up", _vp), ("up_frames", _vp)]


class MapPointsArgs(_c.Structure):
    """pvo_map_points_args"""
    _fields_ = [("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("thresh", _vp),
                ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i), ("min_votes", _i), ("mean_frac", _f),
                ("images", _vp), ("IH", _i), ("IW", _i), ("img_stride", _i), ("img_offset", _i),
                ("labels", _vp), ("reject", _vp), ("LH", _i), ("LW", _i), ("label_div", _i), ("capacity", _i),
                ("xyz", _vp), ("rgba", _vp), ("label", _vp), ("src", _vp), ("frame_start", _vp)]


class TsdfIntegrateArgs(_c.Structure):
    """pvo_tsdf_integrate_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("nz", _i), ("ny", _i), ("nx", _i), ("origin", _f * 3),
                ("voxel", _f), ("trunc", _f), ("z_near", _f), ("w_max", _f),
                ("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("weight", _vp),
                ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i),
                ("images", _vp), ("IH", _i), ("IW", _i), ("img_stride", _i), ("img_offset", _i)]


class TsdfMeshArgs(_c.Structure):
    """pvo_tsdf_mesh_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("nz", _i), ("ny", _i), ("nx", _i), ("origin", _f * 3),
                ("voxel", _f), ("min_weight", _f), ("vcap", _i), ("fcap", _i),
                ("verts", _vp), ("normals", _vp), ("rgba", _vp), ("faces", _vp), ("counts", _vp)]


TSDF_BRICK = 8                             # PVO_TSDF_BRICK


class TsdfSparseAllocateArgs(_c.Structure):
    """pvo_tsdf_sparse_allocate_args"""
    _fields_ = [("grid", _vp), ("coord", _vp), ("bricks", _vp), ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i), ("origin", _f * 3),
                ("voxel", _f), ("trunc", _f), ("z_near", _f), ("margin", _f),
                ("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("weight", _vp),
                ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i)]


class TsdfSparseIntegrateArgs(_c.Structure):
    """pvo_tsdf_sparse_integrate_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("coord", _vp), ("bricks", _vp),
                ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i), ("origin", _f * 3),
                ("voxel", _f), ("trunc", _f), ("z_near", _f), ("w_max", _f),
                ("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("weight", _vp),
                ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i),
                ("images", _vp), ("IH", _i), ("IW", _i), ("img_stride", _i), ("img_offset", _i), ("kept", _vp)]


class TsdfSparseMeshArgs(_c.Structure):
    """pvo_tsdf_sparse_mesh_args"""
    _fields_ = [("grid", _vp), ("coord", _vp), ("bricks", _vp), ("tsdf", _vp), ("wsum", _vp), ("rgb", _vp),
                ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i), ("origin", _f * 3),
                ("voxel", _f), ("min_weight", _f), ("vcap", _i), ("fcap", _i),
                ("verts", _vp), ("normals", _vp), ("rgba", _vp), ("faces", _vp), ("counts", _vp)]


class TsdfPanopticArgs(_c.Structure):
    """pvo_tsdf_panoptic_args"""
    _fields_ = [("label", _vp), ("lconf", _vp), ("labels", _vp), ("lh", _i), ("lw", _i), ("label_div", _i)]


class TsdfMeshLabelsArgs(_c.Structure):
    """pvo_tsdf_mesh_labels_args"""
    _fields_ = [("label", _vp), ("vlabel", _vp)]


_RENDER_TAIL = [("origin", _f * 3), ("voxel", _f), ("min_weight", _f),
                ("poses", _vp), ("intrinsics", _vp), ("ix", _vp), ("N", _i), ("nviews", _i), ("ht", _i), ("wd", _i),
                ("z_near", _f), ("z_far", _f), ("dz", _f),
                ("depth", _vp), ("normal", _vp), ("rgba", _vp), ("out_label", _vp), ("visited", _vp)]


class TsdfRenderArgs(_c.Structure):
    """pvo_tsdf_render_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("label", _vp), ("nz", _i), ("ny", _i), ("nx", _i)] + _RENDER_TAIL


class TsdfSparseRenderArgs(_c.Structure):
    """pvo_tsdf_sparse_render_args"""
    _fields_ = [("grid", _vp), ("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("label", _vp),
                ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i)] + _RENDER_TAIL


TSDF_TRACK_MAX_ITERS = 64                  # PVO_TSDF_TRACK_MAX_ITERS

_TRACK_TAIL = [("origin", _f * 3), ("voxel", _f), ("min_weight", _f),
               ("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("ix", _vp), ("weight", _vp),
               ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i), ("iters", _i), ("min_count", _i),
               ("band", _f), ("huber", _f), ("lm", _f), ("ep", _f),
               ("poses_out", _vp), ("info", _vp), ("system", _vp), ("residual", _vp), ("jac", _vp)]


class TsdfTrackArgs(_c.Structure):
    """pvo_tsdf_track_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("nz", _i), ("ny", _i), ("nx", _i)] + _TRACK_TAIL


class TsdfSparseTrackArgs(_c.Structure):
    """pvo_tsdf_sparse_track_args"""
    _fields_ = [("grid", _vp), ("tsdf", _vp), ("wsum", _vp), ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i)] + _TRACK_TAIL


_REINTEGRATE_TAIL = [("origin", _f * 3), ("voxel", _f), ("trunc", _f), ("z_near", _f), ("w_max", _f), ("w_floor", _f),
                     ("intrinsics", _vp), ("poses_old", _vp), ("disps_old", _vp), ("weight_old", _vp), ("ix_old", _vp),
                     ("poses", _vp), ("disps", _vp), ("weight", _vp), ("ix", _vp),
                     ("N_old", _i), ("N", _i), ("nframes", _i), ("ht", _i), ("wd", _i),
                     ("images", _vp), ("IH", _i), ("IW", _i), ("img_stride", _i), ("img_offset", _i)]


class TsdfReintegrateArgs(_c.Structure):
    """pvo_tsdf_reintegrate_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("nz", _i), ("ny", _i), ("nx", _i)] + _REINTEGRATE_TAIL


class TsdfSparseReintegrateArgs(_c.Structure):
    """pvo_tsdf_sparse_reintegrate_args"""
    _fields_ = [("tsdf", _vp), ("wsum", _vp), ("rgb", _vp), ("coord", _vp), ("bricks", _vp),
                ("gz", _i), ("gy", _i), ("gx", _i), ("cap", _i)] + _REINTEGRATE_TAIL + [("kept", _vp)]


OBJECT_MOTION_MAX_ITERS = 64               # PVO_OBJECT_MOTION_MAX_ITERS


class ObjectMotionArgs(_c.Structure):
    """pvo_object_motion_args"""
    _fields_ = [("poses", _vp), ("disps", _vp), ("intrinsics", _vp), ("labels", _vp), ("ii", _vp), ("jj", _vp), ("target", _vp),
                ("weight", _vp), ("job_edge", _vp), ("job_label", _vp), ("start", _vp),
                ("N", _i), ("E", _i), ("nframes", _i), ("ht", _i), ("wd", _i), ("iters", _i), ("min_count", _i),
                ("z_min", _f), ("huber", _f), ("lm", _f), ("ep", _f),
                ("rel", _vp), ("motion", _vp), ("info", _vp), ("system", _vp), ("centroid", _vp), ("residual", _vp), ("jac", _vp)]


SEGMENT_ASSOC_MAX_S = 1024                 # PVO_SEGMENT_ASSOC_MAX_S


class SegmentAssocArgs(_c.Structure):
    """pvo_segment_assoc_args"""
    _fields_ = [("labels", _vp), ("ii", _vp), ("jj", _vp), ("target", _vp), ("valid", _vp), ("cls", _vp),
                ("E", _i), ("nframes", _i), ("ht", _i), ("wd", _i), ("S", _i), ("min_iou", _f), ("form", _i),
                ("overlap", _vp), ("area_i", _vp), ("area_j", _vp), ("match", _vp), ("match_n", _vp), ("match_d", _vp)]


TRANSPORT_MAX_LEVELS = 8                   # PVO_TRANSPORT_MAX_LEVELS
TRANSPORT_NEAREST, TRANSPORT_REFERENCE = 0, 1


class TransportLevel(_c.Structure):
    """pvo_transport_level"""
    _fields_ = [("ref", _vp), ("cur", _vp), ("out", _vp), ("src", _vp), ("H", _i), ("W", _i), ("sx", _f), ("sy", _f)]


class FeatureTransportArgs(_c.Structure):
    """pvo_feature_transport_args"""
    _fields_ = [("flow", _vp), ("Hf", _i), ("Wf", _i), ("depth", _vp), ("Hd", _i), ("Wd", _i), ("rel_pose", _vp), ("intrinsics", _vp),
                ("C", _i), ("dtype", _i), ("L", _i), ("mode", _i), ("order", _i), ("alpha", _f),
                ("level", TransportLevel * TRANSPORT_MAX_LEVELS)]


PVO_OP_CONV128_WIDE, PVO_OP_SINGLE_STREAM, PVO_OP_ENC_SIDE_STREAM = 1, 2, 4
PVO_KNOB_BA_SOLVER, PVO_KNOB_HEADS_GATHER_FLAT, PVO_KNOB_NO_RIDERS, PVO_KNOB_POST_SEPARATE = 0, 1, 2, 3
PVO_KNOB_EDGE_BLOCKS = 4        # 0 shipped | 1 off | 2 + bits (third, low, agg, trunk): 2 ... 17

_lib = None


class PvoHipError(RuntimeError):
    pass


def load():
    """Load libpvo_hip.so, binding every symbol of the header. Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PvoHipError(
            "libpvo_hip.so not found at %s - build it with `python -m pvo_amd.build` "
            "(there is no CPU fallback)" % LIB_PATH)
    # PyTorch first: its wheel carries its own libamdhip64, and the streams / pointers this module passes into the library
    # are that runtime's.  Loaded before torch, libpvo_hip.so would bind the system ROCm's copy instead - two HIP runtimes
    # in one process, and every launch on a torch stream fails (seen as "HIP launch error" on the first call).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.pvo_version() != PVO_ABI_VERSION or lib.pvo_graph_update_args_size() != ctypes.sizeof(GraphUpdateArgs):
        raise PvoHipError("libpvo_hip.so is ABI version %d with a %d-byte pvo_graph_update_args; this binding is written for version %d / %d bytes - "
                          "rebuild with `python -m pvo_amd.build`" % (lib.pvo_version(), lib.pvo_graph_update_args_size(), PVO_ABI_VERSION,
                                                                     ctypes.sizeof(GraphUpdateArgs)))
    if lib.pvo_map_points_args_size() != ctypes.sizeof(MapPointsArgs):
        raise PvoHipError("libpvo_hip.so has a %d-byte pvo_map_points_args; this binding is written for %d bytes - rebuild with "
                          "`python -m pvo_amd.build`" % (lib.pvo_map_points_args_size(), ctypes.sizeof(MapPointsArgs)))
    for fn, struct in ((lib.pvo_tsdf_integrate_args_size, TsdfIntegrateArgs), (lib.pvo_tsdf_mesh_args_size, TsdfMeshArgs),
                       (lib.pvo_tsdf_sparse_allocate_args_size, TsdfSparseAllocateArgs),
                       (lib.pvo_tsdf_sparse_integrate_args_size, TsdfSparseIntegrateArgs),
                       (lib.pvo_tsdf_sparse_mesh_args_size, TsdfSparseMeshArgs),
                       (lib.pvo_tsdf_panoptic_args_size, TsdfPanopticArgs), (lib.pvo_tsdf_mesh_labels_args_size, TsdfMeshLabelsArgs),
                       (lib.pvo_tsdf_render_args_size, TsdfRenderArgs), (lib.pvo_tsdf_sparse_render_args_size, TsdfSparseRenderArgs),
                       (lib.pvo_tsdf_track_args_size, TsdfTrackArgs), (lib.pvo_tsdf_sparse_track_args_size, TsdfSparseTrackArgs),
                       (lib.pvo_tsdf_reintegrate_args_size, TsdfReintegrateArgs),
                       (lib.pvo_tsdf_sparse_reintegrate_args_size, TsdfSparseReintegrateArgs),
                       (lib.pvo_object_motion_args_size, ObjectMotionArgs), (lib.pvo_segment_assoc_args_size, SegmentAssocArgs),
                       (lib.pvo_feature_transport_args_size, FeatureTransportArgs)):
        if fn() != ctypes.sizeof(struct):
            raise PvoHipError("libpvo_hip.so has a %d-byte %s; this binding is written for %d bytes - rebuild with "
                              "`python -m pvo_amd.build`" % (fn(), struct.__doc__, ctypes.sizeof(struct)))
    _lib = lib
    return lib


PROBE_LIB_PATH = os.path.join(_HERE, "libpvo_probe.so")
PROBE_SIGNATURES = {                       # include/pvo_probe.h
    "pvo_clock_probe": (_i, [_vp, _i, _vp]),
    "pvo_mem_probe": (_c.c_longlong, [_vp, _sz, _i, _i, _i, _vp, _vp]),
}
_probe_lib = None


def load_probe():
    """libpvo_probe.so: the measurement kernels of bench.py / tools (not part of the product library)"""
    global _probe_lib
    if _probe_lib is None:
        load()                                            # (torch's HIP runtime first, as above)
        if not os.path.exists(PROBE_LIB_PATH):
            raise PvoHipError("libpvo_probe.so not found at %s - build it with `python -m pvo_amd.build`" % PROBE_LIB_PATH)
        lib = ctypes.CDLL(PROBE_LIB_PATH)
        for name, (res, args) in PROBE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _probe_lib = lib
    return _probe_lib


def check(status, what):
    if status != 0:
        msg = load().pvo_strerror(status).decode()
        if status == 2:                                   # PVO_ELAUNCH: say which HIP error
            msg += " - " + load().pvo_last_hip_error().decode()
        raise PvoHipError("%s failed: %s (status %d)" % (what, msg, status))
