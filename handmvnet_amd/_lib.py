"""ctypes binding of libhandmv.so (include/handmv.h).  There is deliberately no fallback:
if the HIP extension is missing or cannot be loaded, importing the product path fails."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMV_LIB") or os.path.join(_HERE, "libhandmv.so")   # HMV_LIB: A/B-test another build

# every symbol include/handmv.h declares
SYMBOLS = ["hmv_create", "hmv_set_tensor", "hmv_finalize_weights", "hmv_workspace_bytes", "hmv_reserve", "hmv_forward",
           "hmv_last_error", "hmv_destroy", "hmv_set_capture", "hmv_read_stage", "hmv_set_profiling", "hmv_profile_count",
           "hmv_profile_get", "hmv_op_conv2d", "hmv_op_conv2d_ex", "hmv_op_conv2d_f16", "hmv_op_conv2d_sel", "hmv_op_conv2d_rd", "hmv_op_conv2d_as", "hmv_op_attention", "hmv_op_attention_lq", "hmv_bench_conv", "hmv_pose_metrics", "hmv_forward_frames",
           "hmv_op_prepare_frames", "hmv_set_graphs", "hmv_graph_stats", "hmv_version", "hmv_tile_rule", "hmv_profile_get_bytes", "hmv_poison_workspace", "hmv_launch_count", "hmv_set_tail_fusion", "hmv_set_chain_fusion", "hmv_set_hr_fusion", "hmv_op_conv2d_x3", "hmv_op_hr_fuse_up", "hmv_op_attention_x3",
           "hmv_range_status", "hmv_op_target_heatmaps", "hmv_project_joints", "hmv_pose_losses", "hmv_pose_losses_scratch_bytes",
           "hmv_eval_state_doubles", "hmv_eval_add", "hmv_forward_views", "hmv_op_attention_views", "hmv_pose_losses_views",
           "hmv_eval_add_views", "hmv_forward_frames_views", "hmv_op_next_crop_boxes", "hmv_forward_frames_track",
           "hmv_forward_frames_views_track", "hmv_op_labels_to_windows", "hmv_op_mka", "hmv_seq_eval_sums_doubles",
           "hmv_seq_eval_history_floats", "hmv_seq_eval_add", "hmv_forward_subsets", "hmv_set_attention_capture", "hmv_attention_shape",
           "hmv_read_attention", "hmv_op_attention_probs", "hmv_eval_breakdown_doubles", "hmv_eval_record_floats",
           "hmv_eval_breakdown_add", "hmv_op_hand_ik", "hmv_op_rigid_unapply", "hmv_op_prepare_frames_occluded",
           "hmv_forward_frames_occlusions", "hmv_forward_orders", "hmv_op_pose_consensus", "hmv_op_triangulate",
           "hmv_op_heatmap_peaks", "hmv_op_confidence_select", "hmv_op_input_layout", "hmv_op_maxpool", "hmv_op_soft_argmax",
           "hmv_op_sample_gather", "hmv_op_sample_blend", "hmv_op_tokens_finalize", "hmv_op_layernorm", "hmv_op_splitk_reduce",
           "hmv_op_splitk_layernorm", "hmv_op_add_pe", "hmv_op_cheb_mix", "hmv_eval_absolute_doubles", "hmv_eval_absolute_add",
           "hmv_op_reproject_crop_boxes", "hmv_op_ff_block", "hmv_op_cheb_fused", "hmv_mano_pack_bytes", "hmv_op_mano_pack",
           "hmv_op_mano_skin", "hmv_op_attention_pairs", "hmv_op_conv2d_form", "hmv_eval_vertices_doubles",
           "hmv_eval_vertices_scratch_bytes", "hmv_eval_vertices_add"]

HMV_OK = 0
HMV_ERR_ARG = 1
HMV_ERR_STATE = 2
HMV_ERR_RANGE = 7   # a value outside the fp16 range of its mode (include/handmv.h: "Range contract")


class HmvConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("backbone", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("channels", ctypes.c_int32 * 4), ("num_views", ctypes.c_int32), ("height", ctypes.c_int32),
                ("width", ctypes.c_int32), ("image_size", ctypes.c_int32), ("heatmap_size", ctypes.c_int32),
                ("pos_enc", ctypes.c_int32), ("fusion_layers", ctypes.c_int32), ("decoder", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("device", ctypes.c_int32), ("fusion", ctypes.c_int32)]


class HmvLossArgs(ctypes.Structure):
    """hmv_loss_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("hm_h", ctypes.c_int32),
                ("hm_w", ctypes.c_int32), ("image_size", ctypes.c_int32), ("sigma", ctypes.c_int32), ("root_idx", ctypes.c_int32),
                ("mask_invisible_joints", ctypes.c_int32), ("with_projection", ctypes.c_int32),
                ("w_heatmap", ctypes.c_float), ("w_joints_2d", ctypes.c_float), ("w_joints_3d", ctypes.c_float),
                ("w_g2d", ctypes.c_float), ("w_p2d", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("pred_heatmap", ctypes.c_void_p), ("target_heatmap", ctypes.c_void_p), ("pred_joints_2d", ctypes.c_void_p),
                ("gt_joints_2d", ctypes.c_void_p), ("joints_mask", ctypes.c_void_p), ("pred_joints_cam", ctypes.c_void_p),
                ("gt_joints_cam", ctypes.c_void_p), ("root_joint", ctypes.c_void_p), ("intrinsic", ctypes.c_void_p),
                ("extrinsic", ctypes.c_void_p), ("bbox", ctypes.c_void_p), ("projected", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t)]


class HmvEvalArgs(ctypes.Structure):
    """hmv_eval_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("thr_min", ctypes.c_float), ("thr_max", ctypes.c_float),
                ("pred_joints_cam", ctypes.c_void_p), ("gt_joints_cam", ctypes.c_void_p), ("pred_joints_2d", ctypes.c_void_p),
                ("gt_joints_2d", ctypes.c_void_p), ("joints_mask", ctypes.c_void_p), ("loss_result", ctypes.c_void_p),
                ("state", ctypes.c_void_p), ("state_doubles", ctypes.c_size_t)]


class HmvEvalBreakdownArgs(ctypes.Structure):
    """hmv_eval_breakdown_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("thr_min", ctypes.c_float), ("thr_max", ctypes.c_float),
                ("pred_joints_cam", ctypes.c_void_p), ("gt_joints_cam", ctypes.c_void_p), ("pred_joints_2d", ctypes.c_void_p),
                ("gt_joints_2d", ctypes.c_void_p), ("joints_mask", ctypes.c_void_p), ("view_present", ctypes.c_void_p),
                ("state", ctypes.c_void_p), ("state_doubles", ctypes.c_size_t), ("records", ctypes.c_void_p),
                ("record_capacity", ctypes.c_int64), ("record_base", ctypes.c_int64)]


class HmvEvalAbsoluteArgs(ctypes.Structure):
    """hmv_eval_absolute_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("v_checked", ctypes.c_int32),
                ("pred_joints_cam", ctypes.c_void_p), ("joints_tri", ctypes.c_void_p), ("tri_status", ctypes.c_void_p),
                ("gt_joints_cam", ctypes.c_void_p), ("gt_root", ctypes.c_void_p), ("reproj_err", ctypes.c_void_p),
                ("inliers", ctypes.c_void_p), ("state", ctypes.c_void_p), ("state_doubles", ctypes.c_size_t)]


class HmvEvalVerticesArgs(ctypes.Structure):
    """hmv_eval_vertices_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("n_verts", ctypes.c_int32), ("steps", ctypes.c_int32),
                ("thr_min", ctypes.c_float), ("thr_max", ctypes.c_float), ("unit_div", ctypes.c_float),
                ("pred_vertices", ctypes.c_void_p), ("gt_vertices", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("state", ctypes.c_void_p), ("state_doubles", ctypes.c_size_t), ("scratch", ctypes.c_void_p),
                ("scratch_bytes", ctypes.c_size_t), ("records", ctypes.c_void_p), ("record_capacity", ctypes.c_int64),
                ("record_base", ctypes.c_int64)]


class HmvSeqEvalArgs(ctypes.Structure):
    """hmv_seq_eval_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("pred_joints_cam", ctypes.c_void_p), ("gt_joints_cam", ctypes.c_void_p), ("track_status", ctypes.c_void_p),
                ("slot_info", ctypes.c_void_p), ("restart", ctypes.c_void_p), ("sums", ctypes.c_void_p), ("history", ctypes.c_void_p),
                ("sums_doubles", ctypes.c_size_t), ("history_floats", ctypes.c_size_t)]


class HmvConsensusArgs(ctypes.Structure):
    """hmv_consensus_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("S", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32),
                ("target_cam", ctypes.c_int32), ("mode", ctypes.c_int32), ("iterations", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("poses", ctypes.c_void_p), ("ref_cam", ctypes.c_void_p), ("extrinsic", ctypes.c_void_p), ("aligned", ctypes.c_void_p),
                ("consensus", ctypes.c_void_p), ("spread", ctypes.c_void_p), ("deviation", ctypes.c_void_p)]


class HmvTriangulateArgs(ctypes.Structure):
    """hmv_triangulate_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("J", ctypes.c_int32),
                ("S", ctypes.c_int32), ("n_cams", ctypes.c_int32), ("image_size", ctypes.c_int32), ("extrinsic_kind", ctypes.c_int32),
                ("refit", ctypes.c_int32), ("threshold", ctypes.c_float),
                ("points", ctypes.c_void_p), ("bbox", ctypes.c_void_p), ("intrinsic", ctypes.c_void_p), ("extrinsic", ctypes.c_void_p),
                ("present", ctypes.c_void_p), ("joint_mask", ctypes.c_void_p), ("subsets", ctypes.c_void_p), ("frame_cam", ctypes.c_void_p),
                ("points3d", ctypes.c_void_p), ("reproj_err", ctypes.c_void_p), ("inliers", ctypes.c_void_p), ("winner", ctypes.c_void_p),
                ("status", ctypes.c_void_p)]


class HmvPeaksArgs(ctypes.Structure):
    """hmv_peaks_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("N", ctypes.c_int32), ("J", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32),
                ("heatmap", ctypes.c_void_p), ("maxval", ctypes.c_void_p), ("index", ctypes.c_void_p), ("preds", ctypes.c_void_p)]


class HmvConfidenceSelectArgs(ctypes.Structure):
    """hmv_confidence_select_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("J", ctypes.c_int32),
                ("carry", ctypes.c_int32), ("threshold", ctypes.c_double), ("step", ctypes.c_double),
                ("conf", ctypes.c_void_p), ("present", ctypes.c_void_p), ("joint_mask", ctypes.c_void_p), ("mask_out", ctypes.c_void_p),
                ("level", ctypes.c_void_p), ("lowered", ctypes.c_void_p), ("selected", ctypes.c_void_p)]


class HmvReprojectBoxesArgs(ctypes.Structure):
    """hmv_reproject_boxes_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("margin", ctypes.c_int32),
                ("square", ctypes.c_int32), ("require_all", ctypes.c_int32),
                ("points3d", ctypes.c_void_p), ("point_status", ctypes.c_void_p), ("frame_cam", ctypes.c_void_p),
                ("intrinsic", ctypes.c_void_p), ("extrinsic", ctypes.c_void_p), ("joints_img", ctypes.c_void_p),
                ("crop_boxes", ctypes.c_void_p), ("bbox", ctypes.c_void_p), ("status", ctypes.c_void_p), ("source", ctypes.c_void_p),
                ("joints_reproj", ctypes.c_void_p), ("gap", ctypes.c_void_p)]


class HmvFfBlockArgs(ctypes.Structure):
    """hmv_ff_block_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("rows", ctypes.c_int32), ("d", ctypes.c_int32), ("ld", ctypes.c_int32),
                ("hid", ctypes.c_int32), ("S", ctypes.c_int32), ("lds", ctypes.c_int32), ("ldr", ctypes.c_int32),
                ("slice", ctypes.c_int64), ("rg_out", ctypes.c_int32), ("rg_in", ctypes.c_int32), ("ldx", ctypes.c_int32),
                ("ldw1", ctypes.c_int32), ("ldw2", ctypes.c_int32), ("ldo", ctypes.c_int32), ("tile_rows", ctypes.c_int32),
                ("tile_rows_used", ctypes.c_int32),
                ("slab", ctypes.c_void_p), ("bias0", ctypes.c_void_p), ("res", ctypes.c_void_p), ("x", ctypes.c_void_p),
                ("n1g", ctypes.c_void_p), ("n1b", ctypes.c_void_p), ("fg", ctypes.c_void_p), ("fb", ctypes.c_void_p),
                ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("n2g", ctypes.c_void_p), ("n2b", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_pairs", ctypes.c_void_p),
                ("sat", ctypes.c_void_p)]


class HmvChebFusedArgs(ctypes.Structure):
    """hmv_cheb_fused_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("B", ctypes.c_int32), ("K", ctypes.c_int32), ("ldx", ctypes.c_int32),
                ("c1", ctypes.c_int32), ("ldw1", ctypes.c_int32), ("c2", ctypes.c_int32), ("ldw2", ctypes.c_int32),
                ("c3", ctypes.c_int32), ("ldw3", ctypes.c_int32), ("ldo", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("x", ctypes.c_void_p), ("w1", ctypes.c_void_p), ("bias1", ctypes.c_void_p), ("w2", ctypes.c_void_p),
                ("bias2", ctypes.c_void_p), ("w3", ctypes.c_void_p), ("bias3", ctypes.c_void_p), ("tk", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p), ("out", ctypes.c_void_p)]


HMV_FORM_DUAL, HMV_FORM_CHAIN, HMV_FORM_POOL, HMV_FORM_PHASES, HMV_FORM_SPLITK, HMV_FORM_PAIR_OUT = 1, 2, 4, 8, 16, 32
ROUTE_RULE, ROUTE_NEVER, ROUTE_FORCE = 0, 1, 2   # the route_* fields of hmv_conv_form_args


class HmvConvFormArgs(ctypes.Structure):
    """hmv_conv_form_args of include/handmv.h."""
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "struct_size", "dtype", "form", "N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "relu", "Ho", "Wo",
        "ld_in", "ldc", "ldr", "ld_in2", "route_stream", "route_gemm8", "route_hs", "route_x3k16", "gemm8_persist",
        "Cin2", "H2", "W2", "stride2", "next_cout", "pool_h", "pool_w", "merged", "slices", "reserved")] +
                [(n, ctypes.c_void_p) for n in ("in_", "residual", "in2", "w", "bias", "w2", "bias2", "next_w", "next_bias",
                                                "out", "next_out")] + [("kernel_name", ctypes.c_char_p)])


MANO_BETAS_NONE, MANO_BETAS_SHARED, MANO_BETAS_PER_ROW = 0, 1, 2   # HMV_MANO_BETAS_* of include/handmv.h


class HmvManoParams(ctypes.Structure):
    """hmv_mano_params of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("n_verts", ctypes.c_int32), ("tips", ctypes.c_int32 * 5), ("reserved", ctypes.c_int32),
                ("v_template", ctypes.c_void_p), ("shapedirs", ctypes.c_void_p), ("posedirs", ctypes.c_void_p),
                ("J_regressor", ctypes.c_void_p), ("weights", ctypes.c_void_p)]


class HmvManoSkinArgs(ctypes.Structure):
    """hmv_mano_skin_args of include/handmv.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("n", ctypes.c_int32), ("n_verts", ctypes.c_int32), ("betas_mode", ctypes.c_int32),
                ("project", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("packed", ctypes.c_void_p), ("rot", ctypes.c_void_p), ("betas", ctypes.c_void_p), ("align", ctypes.c_void_p),
                ("vertices", ctypes.c_void_p), ("joints", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class HandMvError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Loads libhandmv.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HandMvError(f"{LIB_PATH} is missing: build it with `python -m handmvnet_amd.build` "
                          "(hipcc --offload-arch=gfx950). handmvnet_amd has no non-HIP fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, fp = ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p
    lib.hmv_create.argtypes = [ctypes.POINTER(HmvConfig), ctypes.POINTER(vp)]
    lib.hmv_set_tensor.argtypes = [vp, ctypes.c_char_p, fp, ctypes.POINTER(ctypes.c_int64), ci]
    lib.hmv_finalize_weights.argtypes = [vp]
    lib.hmv_workspace_bytes.argtypes = [vp, ci]
    lib.hmv_workspace_bytes.restype = ctypes.c_size_t
    lib.hmv_reserve.argtypes = [vp, ci]
    lib.hmv_poison_workspace.argtypes = [vp, ci, vp]
    lib.hmv_launch_count.argtypes = [vp]
    lib.hmv_range_status.argtypes = [vp, ctypes.POINTER(ci), vp]
    lib.hmv_range_status.restype = ctypes.c_int
    lib.hmv_set_tail_fusion.argtypes = [vp, ci]
    lib.hmv_set_chain_fusion.argtypes = [vp, ci]
    lib.hmv_set_hr_fusion.argtypes = [vp, ci]
    lib.hmv_forward.argtypes = [vp, ci, fp, fp, fp, fp, fp, fp, vp]
    lib.hmv_forward_views.argtypes = [vp, ci, ctypes.POINTER(ci), fp, fp, fp, fp, fp, fp, vp]
    lib.hmv_forward_views.restype = ctypes.c_int
    lib.hmv_forward_subsets.argtypes = [vp, ci, ci, fp, fp, fp, fp, fp, fp, fp, vp]   # (subset_mask: host uint8 [S][V])
    lib.hmv_forward_subsets.restype = ctypes.c_int
    lib.hmv_forward_orders.argtypes = [vp, ci, ci, fp, fp, fp, fp, fp, fp, fp, vp]   # (orders: host int32 [S][V], padded with -1)
    lib.hmv_forward_orders.restype = ctypes.c_int
    lib.hmv_op_pose_consensus.argtypes = [ci, ctypes.POINTER(HmvConsensusArgs), vp]
    lib.hmv_op_pose_consensus.restype = ctypes.c_int
    lib.hmv_op_triangulate.argtypes = [ci, ctypes.POINTER(HmvTriangulateArgs), vp]
    lib.hmv_op_triangulate.restype = ctypes.c_int
    lib.hmv_op_heatmap_peaks.argtypes = [ci, ctypes.POINTER(HmvPeaksArgs), vp]
    lib.hmv_op_heatmap_peaks.restype = ctypes.c_int
    lib.hmv_op_confidence_select.argtypes = [ci, ctypes.POINTER(HmvConfidenceSelectArgs), vp]
    lib.hmv_op_confidence_select.restype = ctypes.c_int
    lib.hmv_op_attention_views.argtypes = [ci, ci, fp, fp, ci, ctypes.POINTER(ci), ci, fp, vp]
    lib.hmv_op_attention_views.restype = ctypes.c_int
    lib.hmv_set_attention_capture.argtypes = [vp, ctypes.c_uint32]
    lib.hmv_set_attention_capture.restype = ctypes.c_int
    lib.hmv_attention_shape.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.hmv_attention_shape.restype = ctypes.c_int
    lib.hmv_read_attention.argtypes = [vp, ci, fp, ctypes.c_size_t, fp, ctypes.c_size_t, vp]
    lib.hmv_read_attention.restype = ctypes.c_int
    lib.hmv_op_attention_probs.argtypes = [ci, ci, fp, fp, ci, ci, ci, ci, ci, ctypes.POINTER(ci), fp, fp, ci, vp]
    lib.hmv_op_attention_probs.restype = ctypes.c_int
    lib.hmv_last_error.argtypes = [vp]
    lib.hmv_last_error.restype = ctypes.c_char_p
    lib.hmv_destroy.argtypes = [vp]
    lib.hmv_destroy.restype = None
    lib.hmv_set_capture.argtypes = [vp, ci]
    lib.hmv_read_stage.argtypes = [vp, ctypes.c_char_p, fp, ctypes.c_size_t, vp]
    lib.hmv_set_profiling.argtypes = [vp, ci]
    lib.hmv_profile_count.argtypes = [vp]
    lib.hmv_profile_get.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                    ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
    lib.hmv_profile_get_bytes.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    lib.hmv_profile_get_bytes.restype = ctypes.c_int
    lib.hmv_op_conv2d.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, vp]
    lib.hmv_op_conv2d_ex.argtypes = [ci, ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, vp]
    lib.hmv_op_conv2d_ex.restype = ctypes.c_int
    lib.hmv_op_conv2d_f16.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, ci, ctypes.POINTER(ctypes.c_char_p), vp]
    lib.hmv_op_conv2d_f16.restype = ctypes.c_int
    lib.hmv_op_conv2d_sel.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, ci, ctypes.POINTER(ctypes.c_char_p), vp]
    lib.hmv_op_conv2d_sel.restype = ctypes.c_int
    lib.hmv_op_conv2d_x3.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, ci, ctypes.POINTER(ctypes.c_char_p), vp]
    lib.hmv_op_conv2d_x3.restype = ctypes.c_int
    lib.hmv_tile_rule.argtypes = [ci, ci, ci, ci, ci]
    lib.hmv_tile_rule.restype = ctypes.c_char_p
    lib.hmv_op_conv2d_rd.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, fp, ci, fp, ci, ctypes.POINTER(ctypes.c_char_p), vp]
    lib.hmv_op_conv2d_rd.restype = ctypes.c_int
    lib.hmv_op_conv2d_as.argtypes = [ci, ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, fp, ci, fp, ci, ci, ci, ctypes.POINTER(ctypes.c_char_p), vp]
    lib.hmv_op_conv2d_as.restype = ctypes.c_int
    lib.hmv_op_attention_lq.argtypes = [ci, fp, ci, ci, fp, fp, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_attention_lq.restype = ctypes.c_int
    lib.hmv_op_attention.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_attention_x3.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_attention_pairs.argtypes = [ci, ci, fp, ci, ci, ci, ci, ci, fp, fp, vp]
    lib.hmv_op_attention_pairs.restype = ctypes.c_int
    lib.hmv_op_hr_fuse_up.argtypes = [ci, ci, fp, ci, ci, ci, ci, ci, ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                      ctypes.POINTER(vp), ctypes.POINTER(vp), ci, vp, vp]
    lib.hmv_op_attention.restype = ctypes.c_int
    lib.hmv_bench_conv.argtypes = [ci] * 13 + [ctypes.POINTER(ctypes.c_float)]
    lib.hmv_bench_conv.restype = ctypes.c_int
    lib.hmv_pose_metrics.argtypes = [ci, fp, fp, ci, ci, ci, ctypes.c_float, ctypes.c_float, ci, ci, fp, fp, vp]
    lib.hmv_pose_metrics.restype = ctypes.c_int
    lib.hmv_op_target_heatmaps.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_target_heatmaps.restype = ctypes.c_int
    lib.hmv_project_joints.argtypes = [ci, fp, ci, ci, ci, fp, fp, fp, fp, vp]
    lib.hmv_project_joints.restype = ctypes.c_int
    lib.hmv_pose_losses.argtypes = [ci, ctypes.POINTER(HmvLossArgs), fp, vp]
    lib.hmv_pose_losses.restype = ctypes.c_int
    lib.hmv_pose_losses_views.argtypes = [ci, ctypes.POINTER(HmvLossArgs), fp, fp, vp]
    lib.hmv_pose_losses_views.restype = ctypes.c_int
    lib.hmv_pose_losses_scratch_bytes.argtypes = [ci, ci]
    lib.hmv_pose_losses_scratch_bytes.restype = ctypes.c_size_t
    lib.hmv_eval_state_doubles.argtypes = [ci]
    lib.hmv_eval_state_doubles.restype = ctypes.c_size_t
    lib.hmv_eval_add.argtypes = [ci, ctypes.POINTER(HmvEvalArgs), vp]
    lib.hmv_eval_add.restype = ctypes.c_int
    lib.hmv_eval_add_views.argtypes = [ci, ctypes.POINTER(HmvEvalArgs), fp, vp]
    lib.hmv_eval_add_views.restype = ctypes.c_int
    lib.hmv_eval_breakdown_doubles.argtypes = [ci, ci]
    lib.hmv_eval_breakdown_doubles.restype = ctypes.c_size_t
    lib.hmv_eval_record_floats.argtypes = [ci]
    lib.hmv_eval_record_floats.restype = ctypes.c_size_t
    lib.hmv_eval_breakdown_add.argtypes = [ci, ctypes.POINTER(HmvEvalBreakdownArgs), vp]
    lib.hmv_eval_breakdown_add.restype = ctypes.c_int
    lib.hmv_eval_absolute_doubles.argtypes = [ci]
    lib.hmv_eval_absolute_doubles.restype = ctypes.c_size_t
    lib.hmv_eval_absolute_add.argtypes = [ci, ctypes.POINTER(HmvEvalAbsoluteArgs), vp]
    lib.hmv_eval_absolute_add.restype = ctypes.c_int
    lib.hmv_eval_vertices_doubles.argtypes = [ci, ci]
    lib.hmv_eval_vertices_doubles.restype = ctypes.c_size_t
    lib.hmv_eval_vertices_scratch_bytes.argtypes = [ci, ci, ci]
    lib.hmv_eval_vertices_scratch_bytes.restype = ctypes.c_size_t
    lib.hmv_eval_vertices_add.argtypes = [ci, ctypes.POINTER(HmvEvalVerticesArgs), vp]
    lib.hmv_eval_vertices_add.restype = ctypes.c_int
    lib.hmv_forward_frames_views.argtypes = [vp, ci, ctypes.POINTER(ci), fp, ci, ci, fp, fp, ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_float), fp, fp, fp, fp, fp, vp]
    lib.hmv_forward_frames_views.restype = ctypes.c_int
    lib.hmv_forward_frames.argtypes = [vp, ci, fp, ci, ci, fp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                       fp, fp, fp, fp, fp, vp]
    lib.hmv_forward_frames.restype = ctypes.c_int
    lib.hmv_op_next_crop_boxes.argtypes = [ci, ci, fp, fp, fp, ci, ci, ci, fp, fp, fp, fp, vp]
    lib.hmv_op_next_crop_boxes.restype = ctypes.c_int
    lib.hmv_forward_frames_track.argtypes = lib.hmv_forward_frames.argtypes[:-1] + [ci, ci, fp, fp, vp]
    lib.hmv_forward_frames_track.restype = ctypes.c_int
    lib.hmv_forward_frames_views_track.argtypes = lib.hmv_forward_frames_views.argtypes[:-1] + [ci, ci, fp, fp, vp]
    lib.hmv_forward_frames_views_track.restype = ctypes.c_int
    lib.hmv_op_reproject_crop_boxes.argtypes = [ci, ctypes.POINTER(HmvReprojectBoxesArgs), vp]
    lib.hmv_op_reproject_crop_boxes.restype = ctypes.c_int
    lib.hmv_op_labels_to_windows.argtypes = [ci, ci, fp, fp, fp, fp, ci, fp, fp, fp, vp]
    lib.hmv_op_labels_to_windows.restype = ctypes.c_int
    lib.hmv_op_mka.argtypes = [ci, fp, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_mka.restype = ctypes.c_int
    lib.hmv_seq_eval_sums_doubles.argtypes = [ci]
    lib.hmv_seq_eval_sums_doubles.restype = ctypes.c_size_t
    lib.hmv_seq_eval_history_floats.argtypes = [ci]
    lib.hmv_seq_eval_history_floats.restype = ctypes.c_size_t
    lib.hmv_seq_eval_add.argtypes = [ci, ctypes.POINTER(HmvSeqEvalArgs), vp]
    lib.hmv_seq_eval_add.restype = ctypes.c_int
    lib.hmv_op_hand_ik.argtypes = [ci, fp, fp, ci, fp, fp, fp, fp, vp]
    lib.hmv_op_hand_ik.restype = ctypes.c_int
    lib.hmv_op_rigid_unapply.argtypes = [ci, fp, fp, ci, ci, fp, vp]
    lib.hmv_op_rigid_unapply.restype = ctypes.c_int
    lib.hmv_mano_pack_bytes.argtypes = [ci]
    lib.hmv_mano_pack_bytes.restype = ctypes.c_size_t
    lib.hmv_op_mano_pack.argtypes = [ci, ctypes.POINTER(HmvManoParams), vp, vp]
    lib.hmv_op_mano_pack.restype = ctypes.c_int
    lib.hmv_op_mano_skin.argtypes = [ci, ctypes.POINTER(HmvManoSkinArgs), vp]
    lib.hmv_op_mano_skin.restype = ctypes.c_int
    lib.hmv_op_prepare_frames.argtypes = [ci, fp, ci, ci, ci, fp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                          ci, ci, fp, vp]
    lib.hmv_op_prepare_frames.restype = ctypes.c_int
    lib.hmv_op_prepare_frames_occluded.argtypes = [ci, fp, ci, ci, ci, fp, fp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                                   ci, ci, fp, vp]
    lib.hmv_op_prepare_frames_occluded.restype = ctypes.c_int
    # (occ_view: host int32 [n_occ]; occ_rects: device int32 [n_occ][batch][4])
    lib.hmv_forward_frames_occlusions.argtypes = [vp, ci, fp, ci, ci, fp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                                  fp, fp, ci, ctypes.POINTER(ci), fp, fp, fp, fp, fp, fp, vp]
    lib.hmv_forward_frames_occlusions.restype = ctypes.c_int
    # the non-GEMM kernels of a forward (every operand a device pointer)
    cf = ctypes.c_float
    lib.hmv_op_input_layout.argtypes = [ci, ci, ci, fp, ci, ci, ci, fp, fp, vp]
    lib.hmv_op_maxpool.argtypes = [ci, ci, fp, ci, ci, ci, ci, fp, vp]
    lib.hmv_op_soft_argmax.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, cf, cf, fp, vp]
    lib.hmv_op_sample_gather.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, fp, vp]
    lib.hmv_op_sample_blend.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, fp, ci, ci, vp]
    lib.hmv_op_tokens_finalize.argtypes = [ci, fp, ci, ci, ci, ci, ci, fp, fp, fp, fp, ci, fp, fp, fp, fp, vp]
    lib.hmv_op_layernorm.argtypes = [ci, fp, ci, ci, ci, fp, fp, fp, ci, fp, fp, fp, vp]
    lib.hmv_op_splitk_reduce.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, fp, ci, vp]
    lib.hmv_op_splitk_layernorm.argtypes = [ci, fp, ci, ci, ci, ci, fp, fp, ci, ci, ci, fp, fp, fp, ci, fp, fp, fp, vp]
    lib.hmv_op_add_pe.argtypes = [ci, fp, ci, ci, ci, fp, ci, fp, fp, ci, vp]
    lib.hmv_op_cheb_mix.argtypes = [ci, fp, ci, ci, ci, fp, fp, ci, fp, ci, vp]
    for name in ("hmv_op_input_layout", "hmv_op_maxpool", "hmv_op_soft_argmax", "hmv_op_sample_gather", "hmv_op_sample_blend",
                 "hmv_op_tokens_finalize", "hmv_op_layernorm", "hmv_op_splitk_reduce", "hmv_op_splitk_layernorm", "hmv_op_add_pe",
                 "hmv_op_cheb_mix"):
        getattr(lib, name).restype = ctypes.c_int
    # the fused tail kernels (struct entries)
    lib.hmv_op_ff_block.argtypes = [ci, ctypes.POINTER(HmvFfBlockArgs), vp]
    lib.hmv_op_ff_block.restype = ctypes.c_int
    lib.hmv_op_cheb_fused.argtypes = [ci, ctypes.POINTER(HmvChebFusedArgs), vp]
    lib.hmv_op_cheb_fused.restype = ctypes.c_int
    lib.hmv_op_conv2d_form.argtypes = [ci, ctypes.POINTER(HmvConvFormArgs), vp]
    lib.hmv_op_conv2d_form.restype = ctypes.c_int
    lib.hmv_set_graphs.argtypes = [vp, ci]
    lib.hmv_set_graphs.restype = ctypes.c_int
    lib.hmv_graph_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    lib.hmv_graph_stats.restype = ctypes.c_int
    lib.hmv_version.restype = ctypes.c_char_p
    for name in ("hmv_create", "hmv_set_tensor", "hmv_finalize_weights", "hmv_reserve", "hmv_forward", "hmv_set_capture",
                 "hmv_read_stage", "hmv_set_profiling", "hmv_profile_count", "hmv_profile_get", "hmv_op_conv2d"):
        getattr(lib, name).restype = ctypes.c_int
    _lib = lib
    return lib


def check(rc: int, handle=None) -> None:
    if rc != HMV_OK:
        msg = load().hmv_last_error(handle)
        raise HandMvError(f"libhandmv error {rc}: {msg.decode() if msg else '?'}")
