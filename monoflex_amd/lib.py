"""ctypes binding of libmonoflex_hip.so (the C ABI declared in include/monoflex_hip.h).

The product path has no CPU fallback: if the library is missing, or an entry point returns an
error code, a RuntimeError is raised with the library's own message.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFX_LIB_PATH") or os.path.join(HERE, "csrc", "libmonoflex_hip.so")      # (MFX_LIB_PATH: another BUILD of the same library, for A/B timing of kernel revisions: tools/*_bench.py)

MFX_F32, MFX_BF16, MFX_F16, MFX_F16X2 = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_DCN_OFFMASK = 0, 1, 2, 3
MAX_SEG = 9

c_int, c_void_p, c_float, c_size_t = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t


class ConvDesc(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("w_frag", c_void_p), ("scale", c_void_p), ("shift", c_void_p), ("res", c_void_p),
                ("y", c_void_p), ("rowmap", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("x_pixstride", c_int), ("Ck", c_int),
                ("kh", c_int), ("kw", c_int), ("stride", c_int), ("pad_h", c_int), ("pad_w", c_int), ("dil_w", c_int),
                ("Ho", c_int), ("Wo", c_int), ("M", c_int), ("Cout", c_int), ("Cout_pad", c_int), ("K_pad", c_int),
                ("ldy", c_int), ("ldres", c_int), ("act", c_int), ("dtype", c_int), ("out_dtype", c_int),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_int64),
                ("stats", c_void_p), ("stats_ncopy", c_int), ("stats_done", ctypes.POINTER(c_int)), ("w_frag_pair", c_void_p)]


class CatDesc(ctypes.Structure):
    _fields_ = [("src", c_void_p * MAX_SEG), ("stride", c_int * MAX_SEG), ("off", c_int * MAX_SEG),
                ("nseg", c_int), ("Cseg", c_int),
                ("w", c_void_p), ("scale", c_void_p), ("shift", c_void_p), ("res", c_void_p), ("y", c_void_p),
                ("M", c_int), ("Cout", c_int), ("Cout_pad", c_int), ("K_pad", c_int), ("ldy", c_int),
                ("ldres", c_int), ("act", c_int), ("dtype", c_int)]


class DcnDesc(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("offmask", c_void_p), ("w", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
                ("y", c_void_p), ("w_frag", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("C", c_int),
                ("kh", c_int), ("kw", c_int), ("stride", c_int), ("pad", c_int), ("dil", c_int),
                ("Ho", c_int), ("Wo", c_int), ("Cout", c_int), ("Cout_pad", c_int), ("K_pad", c_int),
                ("ldy", c_int), ("act", c_int), ("dtype", c_int), ("w_frag_f16", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_int64),
                ("off_w_frag_f16", c_void_p), ("off_shift", c_void_p), ("offmask_out", c_void_p),
                ("nonsquare", c_int), ("stride_w", c_int), ("pad_w", c_int), ("dil_w", c_int), ("w_pair_f16", c_void_p)]


class HeadsDesc(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("w1", c_void_p), ("scale1", c_void_p), ("shift1", c_void_p), ("w2", c_void_p),
                ("bias2", c_void_p), ("out", c_void_p), ("planar", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("nbranch", c_int), ("K_pad", c_int), ("ld_out", c_int),
                ("dtype", c_int), ("planar_c", c_int), ("ch_off", c_int * 16), ("c_out", c_int * 16), ("w2_scale", ctypes.c_float * 16),
                ("w1_32", c_void_p), ("w2_32", c_void_p)]


class EdgeChainDesc(ctypes.Structure):                          # mfx_edge_chain_desc
    _fields_ = [(n, c_void_p) for n in ("x", "edge_xy", "w_trunk", "scale_trunk", "shift_trunk", "w_conv", "scale_conv", "shift_conv",
                                        "w_out", "bias_out", "out")] + \
        [(n, c_int) for n in ("B", "H", "W", "C", "L", "head_conv", "ksize", "relu", "dtype")]


class KittiDesc(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "records", "n_obj", "P", "img_wh", "flip", "hm", "cls_ids", "target_centers", "keypoints", "keypoints_depth_mask",
        "dimensions", "locations", "reg_mask", "reg_weight", "offset_3D", "bboxes", "gt_bboxes", "rotys", "trunc_mask", "alphas",
        "orientations", "occlusions", "truncations", "pad_size", "edge_indices", "edge_len", "P_out", "heat_radius", "status")] + \
        [(n, c_int) for n in ("B", "max_objs", "in_w", "in_h", "down", "num_classes")] + \
        [(n, ctypes.c_double) for n in ("filter_trunc", "filter_size", "edge_ratio")]


class KittiEncodeCfg(ctypes.Structure):
    """mfx_kitti_encode_cfg: the encoder's dataset switches, beside the descriptor."""
    _fields_ = [(n, ctypes.c_int32) for n in ("consider_outside_objs", "adjust_boundary_heatmap", "keypoint_visible_modify",
                                              "heatmap_center_2d")]


class KittiEvalDesc(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("gt", "dt", "gt_off", "dt_off", "pair_off", "classes", "min_overlaps", "overlaps", "tp_scores",
                                        "num_valid_gt", "thresholds", "num_thresholds", "pr")] + \
        [(n, c_int) for n in ("B", "n_gt", "n_dt", "num_classes", "num_k", "compute_aos")] + [("n_pairs", ctypes.c_int64)]


class AdamWDesc(ctypes.Structure):                              # mfx_adamw_desc
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("step", c_void_p), ("numel", ctypes.c_longlong),
                ("group", c_int), ("pad_", c_int)]


class AdamWGroup(ctypes.Structure):                             # mfx_adamw_group
    _fields_ = [("lr", c_void_p), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float)]


class PackDesc(ctypes.Structure):                               # mfx_pack_desc
    _fields_ = [("w", c_void_p), ("packed", c_void_p), ("frag", c_void_p)] + \
        [(n, c_int) for n in ("Cout", "Cin", "kh", "kw", "mode", "rows_pad", "K_pad", "ck")]


HEAD_MAX_BRANCH = 8


class HeadSparseDesc(ctypes.Structure):                         # mfx_head_sparse_desc
    _fields_ = [(n, c_int) for n in ("nbranch", "N", "B", "H", "W", "C", "dtype", "ld_out")] + [("rows", c_void_p)] + \
        [(n, c_void_p * HEAD_MAX_BRANCH) for n in ("y", "mean", "rstd", "gamma", "beta", "w2", "b2")] + \
        [("k", c_int * HEAD_MAX_BRANCH), ("out_off", c_int * HEAD_MAX_BRANCH), ("out", c_void_p), ("dout", c_void_p), ("g", c_void_p)] + \
        [(n, c_void_p * HEAD_MAX_BRANCH) for n in ("sums", "dw2", "db2", "dx")] + [("arena", c_void_p), ("arena_bytes", c_size_t)]


class GramDesc(ctypes.Structure):                               # mfx_gram_desc (csrc/gram_heads.hip)
    _fields_ = [("x", c_void_p), ("rows", c_void_p), ("extra_rows", c_void_p)] + \
        [(n, c_int) for n in ("B", "H", "W", "C", "N", "Ne", "F", "nbranch", "extra_branch", "ld_out", "dtype", "nring", "ring_width", "arena_bytes")] + \
        [("momentum", c_float), ("Mt", c_float)] + \
        [(n, c_void_p * HEAD_MAX_BRANCH) for n in ("wk", "gamma", "beta", "w2", "b2", "run_mean", "run_var", "nbt", "dgamma", "dbeta", "dw2", "db2", "dwt")] + \
        [("eps", c_float * HEAD_MAX_BRANCH), ("k", c_int * HEAD_MAX_BRANCH), ("off", c_int * HEAD_MAX_BRANCH)] + \
        [(n, c_void_p) for n in ("A", "Wkc", "WkT", "R5", "S0", "P", "csA", "G", "m", "Tm", "sums", "stat", "Y", "Ye", "act", "act_e", "out",
                                 "dout", "dact_e", "dYh", "dYl", "dYeh", "dYel", "dsum", "ds", "scal", "Dw16", "dm", "dGs", "Kx", "Gn16", "cscale", "cshift",
                                 "dAf", "dArows", "dx", "ring_inv", "ring_idx", "dwo", "dwe")]


OBJ_ROW, OBJ_TERMS, OBJ_VALUES = 72, 10, 24                    # MFX_OBJ_ROW / MFX_OBJ_TERMS / MFX_OBJ_VALUES


class ObjectLossCfg(ctypes.Structure):                          # mfx_object_loss_cfg
    _fields_ = [("w", c_float * OBJ_TERMS), ("dim_mean", c_float * 9), ("dim_std", c_float * 9), ("dim_weight", c_float * 3),
                ("depth_ref", c_float * 2), ("depth_range", c_float * 2)] + \
        [(n, c_float) for n in ("unc_lo", "unc_hi", "down_ratio", "eps")] + \
        [(n, c_int) for n in ("depth_mode", "has_depth_range", "dim_exp", "dim_use_std", "iou_type", "corner_depth_mode",
                              "separate_trunc", "trunc_log", "modify_invalid")] + [("ch", c_int * 9), ("reg_width", c_int)]
    # the two loss kinds of mfx_object_loss_types travel BESIDE the struct (its layout is fixed): plain Python attributes of this object, not fields
    reg_loss = 0                                                # index into REG_LOSSES
    depth_loss = 0                                              # index into DEPTH_LOSSES


class DecodeCfg(ctypes.Structure):                              # mfx_decode_cfg
    _fields_ = [("dim_mean", c_float * 9), ("dim_std", c_float * 9), ("depth_ref", c_float * 2), ("depth_range", c_float * 2),
                ("down_ratio", c_float), ("eps", c_float)] + \
        [(n, c_int) for n in ("depth_decode", "dim_exp", "dim_use_std", "uncertainty_as_conf", "output_depth")]


class HeadLayout(ctypes.Structure):                             # mfx_head_layout
    _fields_ = [("ch", c_int * 9), ("reg_width", c_int)]


# every symbol include/monoflex_hip.h declares: name -> (restype, argtypes)
_P, _I, _F, _S = c_void_p, c_int, c_float, c_size_t
SYMBOLS = {
    "mfx_abi_version": (_I, []),
    "mfx_last_error": (ctypes.c_char_p, []),
    "mfx_stem_conv7x7_nchw": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_f1_fused": (_I, [_P] * 11 + [_I, _I, _I, _I, _I, _P]),
    "mfx_set_option": (_I, [ctypes.c_char_p, _I]),
    "mfx_reset_options": (_I, []),
    "mfx_commit_options": (_I, []),
    "mfx_get_counter": (ctypes.c_long, [ctypes.c_char_p]),
    "mfx_f16x2_range_check": (ctypes.c_int, [ctypes.c_int]),
    "mfx_dcn_v2_workspace_bytes": (_S, [_I] * 14),
    "mfx_dcn_v2_workspace_bytes_g": (_S, [_I] * 15),
    "mfx_dcn_v2_forward": (_I, [_P] * 6 + [_I] * 14 + [_P, _S, _P]),
    "mfx_dcn_v2_backward": (_I, [_P] * 11 + [_I] * 14 + [_P, _S, _P]),
    "mfx_dcn_v2_psroi_pooling_forward": (_I, [_P] * 5 + [_I] * 8 + [_F] + [_I] * 5 + [_F, _P]),
    "mfx_dcn_v2_psroi_pooling_backward": (_I, [_P] * 7 + [_I] * 8 + [_F] + [_I] * 5 + [_F, _P]),
    "mfx_conv2d_nhwc": (_I, [ctypes.POINTER(ConvDesc), _P]),
    "mfx_cat_conv1x1_nhwc": (_I, [ctypes.POINTER(CatDesc), _P]),
    "mfx_dcn_nhwc": (_I, [ctypes.POINTER(DcnDesc), _P]),
    "mfx_dcn_sample_nhwc": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_project_nhwc": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_maxpool2x2_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "mfx_upsample_add_nhwc": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_nchw_to_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_nhwc_to_nchw": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_pack_image_nhwc4": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_heads_fused": (_I, [ctypes.POINTER(HeadsDesc), _P]),
    "mfx_heads_fused_act": (_I, [ctypes.POINTER(HeadsDesc), _I, _P]),
    "mfx_dcn_fuses_offset_conv": (_I, [ctypes.POINTER(DcnDesc)]),
    "mfx_dcn_module_group": (_I, [ctypes.POINTER(ConvDesc), ctypes.POINTER(DcnDesc), _I, _P]),
    "mfx_edge_scatter_add": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P]),
    "mfx_edge_chain": (_I, [ctypes.POINTER(EdgeChainDesc), _P]),
    "mfx_edge_chain_act": (_I, [ctypes.POINTER(EdgeChainDesc), _I, _P]),
    "mfx_edge_chain_applies": (_I, [ctypes.POINTER(EdgeChainDesc)]),
    "mfx_edge_chain_ks": (_I, [ctypes.POINTER(EdgeChainDesc), _I, _P]),
    "mfx_edge_chain_ks_applies": (_I, [ctypes.POINTER(EdgeChainDesc)]),
    "mfx_decode_topk_workspace_bytes": (_S, [_I, _I, _I]),
    "mfx_decode_topk": (_I, [_P, ctypes.c_long, ctypes.c_long, ctypes.c_long, _I, _I, _I, _I, _I, _P, _P, _P, _S, _P]),
    "mfx_conv_wgrad_nhwc": (_I, [_P, _P, _P] + [_I] * 15 + [_P]),
    "mfx_conv_wgrad_nhwc_dil": (_I, [_P, _P, _P] + [_I] * 16 + [_P]),
    "mfx_conv_wgrad_oihw": (_I, [_P, _P, _P] + [_I] * 17 + [_P, _S, _P]),
    "mfx_pack_conv_weight": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P]),
    "mfx_adamw_chunk_elems": (_I, []),
    "mfx_adamw_multi": (_I, [_P, _P, _I, ctypes.c_longlong, _P, _P, _P]),
    "mfx_optim_multi": (_I, [_P, _P, _I, ctypes.c_longlong, _P, _I, _P, _P, _P]),
    "mfx_optim_multi_sched": (_I, [_P, _P, _I, ctypes.c_longlong, _P, _P, _I, _P, _P, _P]),
    "mfx_grad_norm_workspace_bytes": (_S, [ctypes.c_longlong]),
    "mfx_grad_norm_multi": (_I, [_P, _P, _I, ctypes.c_longlong, _F, _P, _S, _P, _P, _P]),
    "mfx_colsum": (_I, [_P, _P, ctypes.c_long, _I, _I, _I, _P]),
    "mfx_colsum_add": (_I, [_P, _P, ctypes.c_long, _I, _I, _I, _P]),
    "mfx_bn_stats": (_I, [_P, _P, _P, ctypes.c_long, _I, _I, _P]),
    "mfx_bn_finalize": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, ctypes.c_long, _P, _P, _P, _P, _I, _P]),
    "mfx_bn_act_fwd": (_I, [_P, _P, _P, _P, _P, ctypes.c_long, _I, _I, _I, _P]),
    "mfx_bn_act_bwd": (_I, [_P] * 10 + [ctypes.c_long, _I, _I, _I, _P]),
    "mfx_stem_wgrad_bf16": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _S, _P]),
    "mfx_stem_wgrad_16": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _S, _P]),
    "mfx_pack_chunk_elems": (_I, []),
    "mfx_pack_conv_weights_batched": (_I, [_P, _P, _I, ctypes.c_longlong, _I, _P]),
    "mfx_head_sparse_fwd": (_I, [ctypes.POINTER(HeadSparseDesc), _P]),
    "mfx_head_sparse_bwd": (_I, [ctypes.POINTER(HeadSparseDesc), _P]),
    "mfx_gram_heads": (_I, [ctypes.POINTER(GramDesc), _I, _P]),
    "mfx_head_sparse_fwd_act": (_I, [ctypes.POINTER(HeadSparseDesc), _I, _P]),
    "mfx_head_sparse_bwd_act": (_I, [ctypes.POINTER(HeadSparseDesc), _I, _P]),
    "mfx_gram_heads_act": (_I, [ctypes.POINTER(GramDesc), _I, _I, _P]),
    "mfx_bn_train_stats": (_I, [_P] * 6 + [_F, _F, ctypes.c_long, _I, _I, _P, _P, _P, _I, _P]),
    "mfx_bn_scratch_bytes": (_S, []),
    "mfx_bn_ncopy": (_I, [_I]),
    "mfx_bn_train_fwd": (_I, [_P] * 8 + [_F, _F, ctypes.c_long, _I, _I, _I, _P, _P, _P, _I, _P]),
    "mfx_bn_train_bwd": (_I, [_P] * 11 + [ctypes.c_long, _I, _I, _I, _P, _P]),
    "mfx_bn_bwd_reduce": (_I, [_P] * 7 + [ctypes.c_long, _I, _I, _I, _P]),
    "mfx_bn_bwd_apply": (_I, [_P] * 10 + [ctypes.c_long, ctypes.c_long, _I, _I, _I, _P]),
    "mfx_maxpool2x2_bwd_nhwc": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "mfx_bn_onepass_stuck": (_I, [_I]),
    "mfx_upsample_bwd_workspace_bytes": (_S, [_I, _I, _I, _I]),
    "mfx_upsample_bwd_nhwc": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _S, _P]),
    "mfx_upsample_bwd_nhwc_oihw": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _S, _P]),
    "mfx_zero_insert2_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "mfx_dcn_backward_nhwc_workspace_bytes": (_S, [_I] * 10),
    "mfx_dcn_backward_nhwc": (_I, [_P] * 8 + [_I] * 10 + [_P, _S, _P]),
    "mfx_dcn_backward_nhwc_bf16": (_I, [_P] * 8 + [_I] * 10 + [_P, _S, _P]),
    "mfx_dcn_backward_v2_workspace_bytes": (_S, [_I] * 6),
    "mfx_dcn_backward_v2": (_I, [_P] * 8 + [_I] * 6 + [_P, _S, _P]),
    "mfx_dcn_backward_v2_rt": (_I, [_P] * 6 + [_I] + [_P] * 2 + [_I] * 6 + [_P, _S, _P]),
    "mfx_focal_loss": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P]),
    "mfx_object_loss": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, ctypes.POINTER(ObjectLossCfg), _P, _P, _P]),
    "mfx_object_loss_types": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, ctypes.POINTER(ObjectLossCfg), _I, _I, _P, _P, _P]),
    "mfx_object_loss_backward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "mfx_object_loss_backward_width": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "mfx_box3d_iou_pairs": (_I, [_P, _P, _I, _I, _P, _P]),
    "mfx_box_nms": (_I, [_P, _P, _I, _I, _I, _F, _I, _P, _P]),
    "mfx_eval_diagnostics": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _P, _P, ctypes.POINTER(DecodeCfg), ctypes.POINTER(HeadLayout), _I, _P, _P, _P, _P]),
    "mfx_kitti_encode_targets": (_I, [ctypes.POINTER(KittiDesc), _P]),
    "mfx_kitti_encode_targets_views": (_I, [ctypes.POINTER(KittiDesc), _P, _P]),
    "mfx_kitti_encode_targets_cfg": (_I, [ctypes.POINTER(KittiDesc), _P, ctypes.POINTER(KittiEncodeCfg), _P]),
    "mfx_kitti_preprocess_u8": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, ctypes.POINTER(c_float), ctypes.POINTER(c_float), _P]),
    "mfx_kitti_preprocess_u8_bgr": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, ctypes.POINTER(c_float), ctypes.POINTER(c_float), _P]),
    "mfx_kitti_preprocess_u8_indexed": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, ctypes.POINTER(c_float), ctypes.POINTER(c_float), _I, _P]),
    "mfx_kitti_encode_targets_indexed": (_I, [ctypes.POINTER(KittiDesc), _P, ctypes.c_int32, _P, ctypes.POINTER(KittiEncodeCfg), _P]),
    "mfx_kitti_eval_overlaps": (_I, [ctypes.POINTER(KittiEvalDesc), _P]),
    "mfx_kitti_eval_match_pass1": (_I, [ctypes.POINTER(KittiEvalDesc), _P]),
    "mfx_kitti_eval_thresholds": (_I, [ctypes.POINTER(KittiEvalDesc), _P, _P]),
    "mfx_kitti_eval_match_pass2": (_I, [ctypes.POINTER(KittiEvalDesc), _P]),
    "mfx_kitti_eval_pack_count": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mfx_kitti_eval_pack_rows": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "mfx_decode_boxes": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _F, _P, _P, _P, _P]),
    "mfx_decode_boxes_mode": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _F, _I, _P, _P, _P, _P]),
    "mfx_decode_boxes_cfg": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _F, ctypes.POINTER(DecodeCfg), _P, _P, _P, _P, _P]),
    "mfx_decode_boxes_heads": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _F, ctypes.POINTER(DecodeCfg), ctypes.POINTER(HeadLayout),
                                    _P, _P, _P, _P, _P]),
    "mfx_decode_boxes_multi": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _F, ctypes.POINTER(DecodeCfg), ctypes.POINTER(HeadLayout),
                                    ctypes.c_uint32, _P, _I, _P, _P, _P, _P, _P, _P]),
}

# mfx_decode_boxes_mode's depth_mode (include/monoflex_hip.h MFX_DEPTH_*), by the reference's `output_depth` names (detector_infer.py:149-198)
DEPTH_MODES = {"soft": 0, "hard": 1, "mean": 2, "direct": 3, "keypoints_avg": 4, "keypoints_center": 5, "keypoints_02": 6, "keypoints_13": 7}
DEPTH_ORACLE = 8                                                # MFX_DEPTH_ORACLE: the bit of 'oracle' in mfx_decode_boxes_multi's `modes` (no decode mode of its own)

NMS_KINDS = {"2d": 1, "3d": 2}                                  # mfx_box_nms' `kind` (MFX_NMS_2D / MFX_NMS_3D) by TEST.USE_NMS value; 'none' launches nothing
NMS_MAX_ROWS = 128                                              # its K limit

DEPTH_DECODES = {"exp": 0, "linear": 1, "inv_sigmoid": 2}      # mfx_decode_cfg.depth_decode = mfx_object_loss_cfg.depth_mode (anno_encoder.py:124-140)


def head_decode_settings(cfg):
    """The head settings that decide how a regression row becomes a box (reference Anno_Encoder.__init__, anno_encoder.py:25-33,45), read
    from a config ONCE for both users: the loss evaluator (mfx_object_loss_cfg) and the post-processor (mfx_decode_cfg) take them from here,
    so that a model cannot train under one rule and decode under another."""
    H = cfg.MODEL.HEAD
    return dict(depth_mode=H.DEPTH_MODE, depth_range=None if H.DEPTH_RANGE is None else tuple(float(v) for v in H.DEPTH_RANGE),
                depth_ref=tuple(float(v) for v in H.DEPTH_REFERENCE),
                dim_mean=tuple(tuple(float(v) for v in row) for row in H.DIMENSION_MEAN),
                dim_std=tuple(tuple(float(v) for v in row) for row in H.DIMENSION_STD),
                dim_modes=list(H.DIMENSION_REG), down_ratio=cfg.MODEL.BACKBONE.DOWN_RATIO, eps=1e-3)


# The nine regression keys in the order of mfx_object_loss_cfg.ch[] / mfx_head_layout.ch[], with their widths
HEAD_KEYS = ('2d_dim', '3d_offset', 'corner_offset', 'corner_uncertainty', '3d_dim', 'ori_cls', 'ori_offset', 'depth', 'depth_uncertainty')
HEAD_WIDTHS = dict(zip(HEAD_KEYS, (4, 2, 20, 3, 3, 8, 8, 1, 1)))
HEAD_OPTIONAL = ('depth_uncertainty', 'corner_offset', 'corner_uncertainty')
# MODEL.HEAD.LOSS_TYPE entries 1 and 3 as mfx_object_loss_types numbers them (csrc/object_loss_math.h REG_* / DEP_*).  Entry 1: 'L1', or ANY other
# string = F.smooth_l1_loss (reference detector_loss.py:53).  Entry 3: 'berhu' is not served (the reference's Berhu_Loss cannot run), see Loss_Computation.
REG_LOSSES = ('L1', 'smooth_l1')
DEPTH_LOSSES = ('L1', 'log', 'inv_sig')
OPTIM_ADAMW, OPTIM_ADAM_L2 = 0, 1                                # mfx_optim_multi `rule`
OPTIM_ADAM_TRUE_WD = 2                                           # ... and mfx_optim_multi_sched's third
CORNER_DEPTHS = ('direct', 'keypoint_mean', 'soft_combine', 'hard_combine')        # mfx_object_loss_cfg.corner_depth_mode
LOSS_REQUIRED = ('hm_loss', 'bbox_loss', 'depth_loss', 'offset_loss', 'orien_loss', 'dims_loss')
LOSS_OPTIONAL = ('corner_loss', 'trunc_offset_loss', 'keypoint_loss', 'keypoint_depth_loss', 'weighted_avg_depth_loss')


class HeadSet:
    """The head set of a config: which of the reference's regression keys the model predicts and where each starts in the R-wide
    regression row (MODEL.HEAD.REGRESSION_HEADS / REGRESSION_CHANNELS flattened, as Converter_key2channel).  Read ONCE for every user --
    the loss evaluator, the post-processor and the predictor take starts, R and what the set can serve from here, in the spirit of
    head_decode_settings().  `du`, `kp`, `cu`: depth_uncertainty / corner_offset / corner_uncertainty present."""

    def __init__(self, regression_heads, regression_channels):
        names = [n for group in regression_heads for n in group]
        widths = [int(w) for group in regression_channels for w in group]
        if len(names) != len(widths) or [len(g) for g in regression_heads] != [len(g) for g in regression_channels]:
            raise NotImplementedError("head set: REGRESSION_HEADS and REGRESSION_CHANNELS do not pair up: %r / %r" % (regression_heads, regression_channels))
        bad = [n for n in names if n not in HEAD_KEYS] + [n for n in set(names) if names.count(n) > 1]
        if bad:
            raise NotImplementedError("head set: unknown or repeated regression keys %s (known: %s)" % (sorted(set(bad)), ", ".join(HEAD_KEYS)))
        missing = [k for k in HEAD_KEYS if k not in names and k not in HEAD_OPTIONAL]
        if missing:
            raise NotImplementedError("head set %s: the required keys %s are missing" % (names, missing))
        wrong = ["%s(%d)" % (n, w) for n, w in zip(names, widths) if HEAD_WIDTHS[n] != w]
        if wrong:
            raise NotImplementedError("head set: channel counts %s differ from the reference's %s" % (wrong, [HEAD_WIDTHS[n] for n in names]))
        self.names, self.widths = names, widths
        self.starts, start = {}, 0
        for n, w in zip(names, widths):
            self.starts[n] = start
            start += w
        self.R = start
        self.du, self.kp, self.cu = ('depth_uncertainty' in names), ('corner_offset' in names), ('corner_uncertainty' in names)
        if self.cu and not self.kp:
            raise NotImplementedError("head set %s: corner_uncertainty without corner_offset" % (names,))
        self.full = self.du and self.kp and self.cu

    def describe(self):
        return "head set (depth_uncertainty %d, corner_offset %d, corner_uncertainty %d; %d channels)" % (self.du, self.kp, self.cu, self.R)

    def ch(self, key):
        """First channel of `key` in the regression row, -1 when the set does not have it."""
        return self.starts.get(key, -1)

    def corner_depths(self):
        """The CORNER_LOSS_DEPTH values this set can serve (the reference raises on the others)."""
        return CORNER_DEPTHS[:1] + (CORNER_DEPTHS[1:2] if self.kp else ()) + (CORNER_DEPTHS[2:] if self.full else ())

    def output_depths(self):
        """The OUTPUT_DEPTH values this set can serve (detector_infer.py:148-204)."""
        out = ('direct',)
        if self.kp:
            out += ('keypoints_avg', 'keypoints_center', 'keypoints_02', 'keypoints_13')
        if self.cu:
            out += ('soft', 'hard', 'mean', 'oracle')
        return out

    def oracle_columns(self):
        """The single-estimate decodes 'oracle' chooses among: the reference's pred_combined_depths columns (detector_infer.py:177-182)."""
        return (('direct',) if self.du else ()) + ('keypoints_center', 'keypoints_02', 'keypoints_13')

    def has_depth_error(self, output_depth):
        """Whether the reference has an estimated_depth_error under `output_depth` (None otherwise: raw score, eval_utils entries None)."""
        if output_depth == 'direct':
            return self.du
        return self.cu

    def check_corner_depth(self, corner_loss_depth):
        if corner_loss_depth not in self.corner_depths():
            raise NotImplementedError("CORNER_LOSS_DEPTH %r with the %s: this set serves %s"
                                      % (corner_loss_depth, self.describe(), ", ".join(self.corner_depths())))

    def check_output_depth(self, output_depth):
        if output_depth not in self.output_depths():
            raise NotImplementedError("OUTPUT_DEPTH %r with the %s: this set serves %s"
                                      % (output_depth, self.describe(), ", ".join(self.output_depths())))

    def check_loss_names(self, loss_names):
        """LOSS_NAMES the set can serve: the six basic terms always, keypoint_loss iff corner_offset (the reference indexes its weight
        unconditionally), keypoint_depth_loss only with corner_offset, weighted_avg_depth_loss only with corner_uncertainty."""
        names = list(loss_names)
        problems = ["%s is required" % n for n in LOSS_REQUIRED if n not in names]
        problems += ["%s is not a loss of the reference" % n for n in names if n not in LOSS_REQUIRED + LOSS_OPTIONAL]
        if self.kp and 'keypoint_loss' not in names:
            problems.append("keypoint_loss is required with corner_offset")
        if not self.kp:
            problems += ["%s needs corner_offset" % n for n in ('keypoint_loss', 'keypoint_depth_loss') if n in names]
        if not self.cu and 'weighted_avg_depth_loss' in names:
            problems.append("weighted_avg_depth_loss needs corner_offset and corner_uncertainty")
        if problems:
            raise NotImplementedError("LOSS_NAMES %s with the %s: %s" % (names, self.describe(), "; ".join(problems)))

    def layout(self):
        """mfx_head_layout of this set."""
        h = HeadLayout()
        for i, key in enumerate(HEAD_KEYS):
            h.ch[i] = self.ch(key)
        h.reg_width = self.R
        return h


def head_set(cfg):
    """HeadSet of a config's MODEL.HEAD.REGRESSION_HEADS / REGRESSION_CHANNELS."""
    return HeadSet(cfg.MODEL.HEAD.REGRESSION_HEADS, cfg.MODEL.HEAD.REGRESSION_CHANNELS)


def fill_decode_settings(c, s):
    """Write the settings of head_decode_settings() into the fields ObjectLossCfg and DecodeCfg share (dim_mean, dim_std, depth_ref,
    depth_range, down_ratio, eps, dim_exp, dim_use_std); the depth rule's number (DEPTH_DECODES) is returned for the field each struct
    names its own way."""
    for name in ("dim_mean", "dim_std"):
        flat = [v for row in s[name] for v in row]
        if len(flat) > 9:
            raise ValueError("%s: at most three (l, h, w) rows" % name)
        for i, v in enumerate(flat):
            getattr(c, name)[i] = v
    c.depth_ref[0], c.depth_ref[1] = s["depth_ref"]
    c.depth_range[0], c.depth_range[1] = s["depth_range"]
    c.down_ratio, c.eps = float(s["down_ratio"]), float(s["eps"])
    c.dim_exp, c.dim_use_std = int(s["dim_modes"][0] == 'exp'), int(bool(s["dim_modes"][2]))
    return DEPTH_DECODES[s["depth_mode"]]


def decode_cfg(settings, uncertainty_as_conf, output_depth="soft"):
    """mfx_decode_cfg from head_decode_settings() + TEST.UNCERTAINTY_AS_CONFIDENCE + the reference's `output_depth` name."""
    c = DecodeCfg()
    c.depth_decode = fill_decode_settings(c, settings)
    c.uncertainty_as_conf, c.output_depth = int(bool(uncertainty_as_conf)), DEPTH_MODES[output_depth]
    return c


_lib = None


def load():
    """Load the shared library (building it is __graft_entry__.build()'s / build.py's job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libmonoflex_hip.so is missing (%s): run `python -m monoflex_amd.build`; "
                           "the MonoFlex HIP path has no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)            # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.mfx_abi_version() != 3:
        raise RuntimeError("libmonoflex_hip.so ABI version mismatch")
    _lib = lib
    # MFX_OPTIONS="name=value,name=value": library tuning switches for this process (mfx_set_option; A/B sweeps of an unmodified bench.py / training script)
    set_options(os.environ.get("MFX_OPTIONS", ""), "MFX_OPTIONS")
    check(lib.mfx_commit_options(), "mfx_commit_options")      # mfx_reset_options() now restores the values AFTER the environment's switches
    return lib


def set_options(spec, what="set_options"):
    """Set library tuning switches (mfx_set_option; csrc/options.h lists them): `spec` is "name=value,name=value" or a dict.
    Raises with the library's message on an unknown name or a value out of range."""
    lib = load()
    items = spec.items() if isinstance(spec, dict) else (kv.partition("=")[::2] for kv in filter(None, spec.split(",")))
    for k, v in items:
        check(lib.mfx_set_option(k.strip().encode(), int(v)), "%s: %s=%s" % (what, k, v))


def f16x2_range_ok(reset=True):
    """Split-precision mode (MODEL.COMPUTE_DTYPE fp16x2): True if every activation turned into an fp16 (hi, lo) operand pair since the last reset was
    finite and inside fp16's range (|x| <= 65504) -- the mode's one numerical precondition.  Synchronises the device."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    rc = load().mfx_f16x2_range_check(1 if reset else 0)
    if rc < 0:
        check(rc, "mfx_f16x2_range_check")
    return rc == 0


def bn_onepass_ok(reset=True):
    """False if a one-launch BatchNorm (csrc/train_kernels.hip bn_*_onepass_kernel) gave up waiting at its grid barrier since the last reset: its
    workgroups did not all become resident, which needs another PROCESS computing on the same device (or two such launches in flight at once).
    The outputs of that launch are wrong; run with MFX_OPTIONS=bn_onepass=0 in such a setup.  Synchronises the device."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    rc = load().mfx_bn_onepass_stuck(1 if reset else 0)
    if rc < 0:
        check(rc, "mfx_bn_onepass_stuck")
    return rc == 0


def set_deterministic(on=True):
    """Bit-reproducible training steps: the library's reductions run in a fixed order (option "deterministic": single-writer
    partial sums instead of fp32 atomics, fixed-point accumulation of the DCN input gradient) and torch's own scatter-type ops
    (index_add_ behind the edge-fusion gather) take their sorted forms.  Slower (roughly 2-3x on a full-size step); meant for
    tests and debugging -- two runs, eager or replayed from a hipGraph, then agree bit for bit."""
    import torch
    check(load().mfx_set_option(b"deterministic", 1 if on else 0), "set_option(deterministic)")
    torch.use_deterministic_algorithms(bool(on), warn_only=True)
    if on:
        torch.utils.deterministic.fill_uninitialized_memory = False        # (torch.empty need not be NaN-filled: every buffer is written)


def check(rc, what):
    if rc != 0:
        msg = load().mfx_last_error().decode(errors="replace")
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg))
