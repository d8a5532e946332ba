"""ctypes binding of libimvoxel_hip.so (the C-ABI declared in include/imvoxel.h).

The product path fails loudly when the library is missing or a call fails: there is no CPU
fallback anywhere in this package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IVX_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libimvoxel_hip.so')      # (IVX_LIB_PATH: A/B builds of the same ABI, tools/)
_lib = None


class IvxError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ('B', 'D', 'H', 'W', 'Cin', 'Cout', 'KD', 'KH', 'KW', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw',
                 'relu', 'res_mode', 'res_h', 'res_w', 'wgt_layout', 'out_mode', 'res_after_act')] + [('post_scale', C.c_float),
                                                                  ('in_dtype', C.c_int32), ('out_dtype', C.c_int32), ('res_scale', C.c_float),
                                                                  ('wino_operands', C.c_int32)]


class ConvRouteOpts(C.Structure):
    """ivx_conv_route_opts: the model-level switches that bear on the route of a convolution."""
    _fields_ = [(n, C.c_int32) for n in ('winograd', 'winograd_tile', 'wino_operands', 'split')] + [('winograd_min_pos', C.c_int64), ('winograd_2d_min_ch', C.c_int32)]


class ConvRoute(C.Structure):
    """ivx_conv_route: the form a convolution runs in and the descriptor to launch."""
    _fields_ = [(n, C.c_int32) for n in ('form', 'tile', 'wino_candidate', 'split_candidate', 'split_fits', 'prefers_winograd')] + [('run', ConvDesc)]


class AnchorHeadDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ('B', 'H', 'W', 'CH', 'num_anchors', 'num_classes', 'cls_off', 'reg_off', 'dir_off',
                 'nms_pre', 'max_num', 'use_rotate_nms', 'hw_transposed')] + \
               [(n, C.c_float) for n in ('score_thr', 'nms_thr', 'dir_offset', 'dir_limit_offset')]


class ModelCfg(C.Structure):
    """ivx_model_cfg (include/imvoxel.h)."""
    _fields_ = [('neck_type', C.c_int32), ('with_trunk', C.c_int32), ('fpn_channels', C.c_int32), ('neck_out_channels', C.c_int32),
                ('n_voxels', C.c_int32 * 3), ('voxel_size', C.c_float * 3), ('num_classes', C.c_int32), ('n_sizes', C.c_int32),
                ('n_rotations', C.c_int32), ('anchor_range', C.c_float * 6), ('anchor_sizes', C.c_float * 12),
                ('anchor_rotations', C.c_float * 4), ('nms_pre', C.c_int32), ('max_num', C.c_int32), ('use_rotate_nms', C.c_int32),
                ('score_thr', C.c_float), ('nms_thr', C.c_float), ('dir_offset', C.c_float), ('dir_limit_offset', C.c_float),
                ('winograd', C.c_int32), ('winograd_tile', C.c_int32),
                ('fast_n_blocks', C.c_int32 * 3), ('unet_channels', C.c_int32 * 4), ('unet_down_layers', C.c_int32 * 4),
                ('unet_up_layers', C.c_int32 * 3),
                ('head_type', C.c_int32), ('head_classes', C.c_int32), ('head_nms_pre', C.c_int32), ('head_use_rotate_nms', C.c_int32),
                ('head_score_thr', C.c_float), ('head_nms_thr', C.c_float), ('dcn_stages', C.c_int32 * 4), ('layout_head', C.c_int32),
                ('layout_linear_size', C.c_int32), ('wino_operands', C.c_int32), ('trunk_operands', C.c_int32), ('storage', C.c_int32),
                ('sampling', C.c_int32)]


# sampling rule of the unprojection: IVX_SAMPLE_NEAREST (the reference's, the default everywhere) | IVX_SAMPLE_BILINEAR (optional extra mode)
SAMPLING = {'nearest': 0, 'bilinear': 1}


def sampling_id(sampling):
    try:
        return SAMPLING[sampling]
    except (KeyError, TypeError):
        raise ValueError(f"sampling must be 'nearest' or 'bilinear', got {sampling!r}") from None


# what the state of a scene is to ivx_view_coverage_fwd: IVX_STATE_NONE (an empty scene) | _COUNT (int32 view counts) | _WSUM (fp32 weight sums) | _MASK (uint8 valid)
STATE_NONE, STATE_COUNT, STATE_WSUM, STATE_MASK = 0, 1, 2, 3


class BackprojectDesc(C.Structure):
    """ivx_backproject_desc (ivx_backproject_fwd_ex, ivx_backproject_gather_fwd)."""
    _fields_ = [(n, C.c_int32) for n in ('B', 'V', 'FH', 'FW', 'C', 'X', 'Y', 'Z')] + [('voxel_size', C.c_float * 3)] + \
               [(n, C.c_int32) for n in ('feat_dtype', 'mode', 'sampling', 'first')]


class LiftLists(C.Structure):
    """ivx_lift_lists (ivx_backproject_lists_fwd): the slot lists, rows and first flags of a listed lift; the pointers are device addresses."""
    _fields_ = [('S', C.c_int32), ('R', C.c_int32), ('view_slot', C.c_void_p), ('row', C.c_void_p), ('first', C.c_void_p)]


class LiftWeights(C.Structure):
    """ivx_lift_weights (ivx_backproject_weighted_fwd): the per-slot weights, per-sample decays and the weight-sum pool of a weighted listed lift; the
    pointers are device addresses."""
    _fields_ = [('view_weight', C.c_void_p), ('decay', C.c_void_p), ('forget_below', C.c_float), ('wsum', C.c_void_p)]


class LiftMaps(C.Structure):
    """ivx_lift_maps (ivx_backproject_mapped_fwd): the per-slot pixel-weight and depth maps of a mapped lift and the gate around a measured depth; the
    pointers are device addresses."""
    _fields_ = [('pixel_weight', C.c_void_p), ('depth', C.c_void_p), ('behind', C.c_float), ('front', C.c_float)]


class PairIO(C.Structure):
    """ivx_pair_io: device-side scales / amax slots of a convolution on fp16-pair activations (ivx_conv_fwd_pio)."""
    _fields_ = [('in_scale', C.c_void_p), ('res_scale', C.c_void_p), ('res_dtype', C.c_int32), ('out_scale', C.c_void_p), ('amax_in', C.c_void_p),
                ('amax_res', C.c_void_p), ('amax_out', C.c_void_p), ('wbound', C.c_float), ('sbound', C.c_float)]


class BottleneckDesc(C.Structure):
    """ivx_bottleneck_desc."""
    _fields_ = [(n, C.c_int32) for n in ('B', 'H', 'W', 'P')]


class BottleneckIO(C.Structure):
    """ivx_bottleneck_io: scalar blocks of the fused bottleneck's input / output and the bound terms of its three layers."""
    _fields_ = [('in_scale', C.c_void_p), ('amax_in', C.c_void_p), ('out_scale', C.c_void_p), ('amax_out', C.c_void_p), ('wbound', C.c_float * 3),
                ('sbound', C.c_float * 3)]


class SampleMeta(C.Structure):
    """ivx_sample_meta."""
    _fields_ = [('intrinsic', C.c_float * 16), ('extrinsics', C.c_void_p), ('origin', C.c_float * 3), ('img_h', C.c_int32), ('img_w', C.c_int32),
                ('ori_h', C.c_int32)]


class IndoorTailDesc(C.Structure):
    """ivx_indoor_tail_desc."""
    _fields_ = [('B', C.c_int32), ('n_levels', C.c_int32), ('k', C.c_int32 * 4), ('n_classes', C.c_int32), ('n_reg', C.c_int32),
                ('use_rotate_nms', C.c_int32), ('max_num', C.c_int32), ('score_thr', C.c_float), ('nms_thr', C.c_float)]


class TraceRec(C.Structure):
    """ivx_trace_rec."""
    _fields_ = [('step', C.c_int32), ('stage', C.c_int32), ('is3d', C.c_int32), ('ms', C.c_float), ('start_ms', C.c_float), ('flops', C.c_double),
                ('bytes', C.c_double), ('name', C.c_char * 48)]


class PlanInfo(C.Structure):
    """ivx_plan_info (include/imvoxel_lab.h): the byte layout of a cached plan of the model handle."""
    _fields_ = [(n, C.c_int64) for n in ('cam_bytes', 'arena', 'ws_off', 'ws_bytes', 'ws2_off', 'ws2_bytes', 'total', 'scal_off', 'scal_bytes')] + \
               [(n, C.c_int32) for n in ('slot_bytes', 'n_sides', 's0', 's1', 'n_steps', 'n_tensors')]


class PlanStep(C.Structure):
    """ivx_plan_step."""
    _fields_ = [(n, C.c_int32) for n in ('kind', 'in_', 'res', 'out', 'out2', 'fuse_out', 'fuse', 'side', 'join', 'tile', 'pio', 'amax_n', 'amax_in_n',
                                         'n_extra_in', 'n_extra_out')] + \
               [('extra_in', C.c_int32 * 12), ('extra_out', C.c_int32 * 4)] + \
               [(n, C.c_int64) for n in ('split', 'ws', 'amax_out', 'amax_in')] + [('name', C.c_char * 48)]


class PlanTensor(C.Structure):
    """ivx_plan_tensor."""
    _fields_ = [(n, C.c_int64) for n in ('off', 'bytes', 'used', 'slot')] + \
               [(n, C.c_int32) for n in ('first', 'last', 'fmt', 'esz', 'caller_owned', 'boundary')]


class ImagePrepDesc(C.Structure):
    """ivx_image_prep_desc: uint8 HWC frames -> Resize -> Normalize -> Pad (ivx_image_prep_u8)."""
    _fields_ = [(n, C.c_int32) for n in ('src_h', 'src_w', 'src_row_bytes', 'dst_h', 'dst_w', 'pad_h', 'pad_w', 'to_rgb')] + \
               [('mean', C.c_float * 3), ('std', C.c_float * 3)]


LENS_BROWN, LENS_FISHEYE = 0, 1      # ivx_lens.model: OpenCV's 5-coefficient model (k1, k2, p1, p2, k3) | its equidistant fisheye model (k1..k4)
MAP_F32, MAP_U16 = 0, 1              # the element type of a source-size map of ivx_map_prep_lens


class Lens(C.Structure):
    """ivx_lens: a real camera (K, distortion) and the ideal pinhole camera the network input shows (ivx_image_prep_lens_u8 / ivx_map_prep_lens)."""
    _fields_ = [('model', C.c_int32)] + [(n, C.c_double) for n in ('fx', 'fy', 'cx', 'cy')] + [('coef', C.c_double * 5)] + \
               [(n, C.c_double) for n in ('new_fx', 'new_fy', 'new_cx', 'new_cy', 'r2_max')]


class FrameFormat(C.Structure):
    """ivx_frame_format: the pixel layout of a source frame and, for the YUV layouts, the integer matrix (ivx_image_prep_fmt_u8)."""
    _fields_ = [('layout', C.c_int32), ('plane1_row_bytes', C.c_int32), ('plane1_offset', C.c_int64)] + \
               [(n, C.c_int32) for n in ('y_off', 'cy', 'cub', 'cug', 'cvg', 'cvr')]


class ConvPlanRec(C.Structure):
    """ivx_conv_plan_rec (include/imvoxel_lab.h): what the conv planner answers for a descriptor (ivx_conv_plan_query)."""
    _fields_ = [('slice_samples', C.c_int32), ('n_slices', C.c_int32)] + \
               [(n, C.c_int32 * 2) for n in ('samples', 'cfg', 'ksplit', 'tail_ks', 'q_total', 'qa', 'bm')] + \
               [('slice_ws', C.c_int64 * 2), ('ws_bytes', C.c_int64)] + [(n, C.c_int32) for n in ('halo_cfg', 'grouped_tile', 'tile_matches', 'rows_dev_ok')]


def declare_plan_view(L):
    """Argument types of the read-only plan view, on libimvoxel_hip.so or on the CPU restatement of the same ABI (tests)."""
    key = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ivx_model_plan_info.argtypes = key + [C.POINTER(PlanInfo)]
    L.ivx_model_plan_step.argtypes = key + [C.c_int32, C.POINTER(PlanStep)]
    L.ivx_model_plan_tensor.argtypes = key + [C.c_int32, C.POINTER(PlanTensor)]


EXPORTS = ['ivx_conv_plan_query', 'ivx_conv_tile_info', 'ivx_model_plan_info', 'ivx_model_plan_step', 'ivx_model_plan_tensor', 'ivx_bottleneck_proj_supported', 'ivx_bottleneck_proj_pack', 'ivx_bottleneck_proj_fwd_pio', 'ivx_anchor_head_decode', 'ivx_fcos3d_head_decode', 'ivx_nms_rotated_bev', 'ivx_nms_aligned3d', 'ivx_bottleneck_supported', 'ivx_bottleneck_fwd_pio', 'ivx_amax_f32', 'ivx_stem_pool_filter_bytes', 'ivx_stem_pool_pack_filters', 'ivx_stem_pool_out_dims', 'ivx_stem_pool_fwd_pair', 'ivx_conv_winograd_set_variant', 'ivx_ubench_mfma', 'ivx_ubench_copy', 'ivx_version', 'ivx_last_error', 'ivx_conv_out_dims', 'ivx_conv_fwd', 'ivx_conv_fwd_naive', 'ivx_conv_set_tile_override', 'ivx_conv_set_epilogue_mode', 'ivx_conv_set_plan_mode', 'ivx_topk_set_mode', 'ivx_conv_workspace_bytes', 'ivx_conv_fwd_ws', 'ivx_conv_set_halo_mode', 'ivx_bf16_pair_split', 'ivx_f16_pair_split', 'ivx_conv_pair_supported', 'ivx_bf16_pair_pack_filters', 'ivx_conv_route', 'ivx_conv_pio_workspace_bytes', 'ivx_conv_fwd_pio', 'ivx_conv_fwd_pio_naive', 'ivx_pair_pack_filters', 'ivx_nchw_to_nhwc_amax', 'ivx_maxpool2d_fwd_pair', 'ivx_f16_pair_merge', 'ivx_model_calibrate_fp8', 'ivx_model_calibrate_fp8_ex', 'ivx_amax_bf16', 'ivx_conv_winograd_output_blocks', 'ivx_conv_winograd_issued_fraction', 'ivx_conv_winograd_output_amax', 'ivx_conv_winograd_input_amax', 'ivx_conv_winograd_fused_supported', 'ivx_conv_winograd_fused_blocks', 'ivx_conv_winograd_gemm_output_amax',
           'ivx_conv_winograd_bg_supported', 'ivx_conv_winograd_bg_bytes', 'ivx_conv_winograd_bg_layer_offset', 'ivx_conv_winograd_bg_plan',
           'ivx_conv_winograd_input_bg', 'ivx_conv_winograd_gemm_bg', 'ivx_conv_winograd_output_bg',
           'ivx_conv_winograd_supported', 'ivx_conv_winograd_weight_elems', 'ivx_conv_winograd_weights', 'ivx_conv_winograd_workspace_bytes',
           'ivx_conv_winograd_input', 'ivx_conv_winograd_gemm', 'ivx_conv_winograd_output', 'ivx_conv_winograd_fwd',
           'ivx_maxpool2d_fwd', 'ivx_maxpool2d_fwd_bf16', 'ivx_maxpool2d_fwd_fp8', 'ivx_global_avgpool_fwd', 'ivx_global_avgpool_fwd_bf16', 'ivx_upsample_trilinear2x_fwd', 'ivx_dcn_im2col_fwd', 'ivx_dcn_im2col_fwd_bf16', 'ivx_dcn_im2col_fwd_pair', 'ivx_nchw_to_nhwc', 'ivx_image_s2d_bf16', 'ivx_nhwc_to_nchw', 'ivx_backproject_mean_fwd', 'ivx_backproject_mean_fwd_amax', 'ivx_backproject_amax_blocks', 'ivx_backproject_mean_fwd_bf16', 'ivx_upsample_trilinear2x_fwd_bf16', 'ivx_backproject_sum_fwd', 'ivx_volume_normalize_fwd',
           'ivx_backproject_accum_fwd', 'ivx_backproject_accum_fwd_bf16', 'ivx_volume_mean_fwd', 'ivx_backproject_fwd_ex', 'ivx_backproject_gather_fwd',
           'ivx_backproject_lists_fwd', 'ivx_backproject_weighted_fwd', 'ivx_volume_wmean_fwd', 'ivx_volume_scroll_fwd', 'ivx_backproject_mapped_fwd',
           'ivx_view_coverage_fwd', 'ivx_volume_warp_fwd', 'ivx_volume_merge_fwd', 'ivx_volume_pack_scratch_bytes', 'ivx_volume_pack_fwd', 'ivx_volume_unpack_fwd',
           'ivx_volume_match_scratch_bytes', 'ivx_volume_match_fwd', 'ivx_volume_align_scratch_bytes', 'ivx_volume_align_fwd',
           'ivx_anchor_head_workspace_bytes', 'ivx_anchor_head_get_bboxes', 'ivx_fcos_head_workspace_bytes',
           'ivx_fcos_head_level_candidates', 'ivx_nms_workspace_bytes',
           'ivx_nms_bev', 'ivx_boxes_overlap_bev', 'ivx_aligned_3d_nms', 'ivx_aligned_3d_nms_workspace_bytes', 'ivx_aligned_3d_nms_ws', 'ivx_multiclass_nms_workspace_bytes', 'ivx_multiclass_nms_bev',
           'ivx_create', 'ivx_destroy', 'ivx_weights_load', 'ivx_weights_finalize', 'ivx_model_workspace_bytes', 'ivx_model_forward',
           'ivx_backbone_fpn_workspace_bytes', 'ivx_backbone_fpn_fwd', 'ivx_neck3d_workspace_bytes', 'ivx_neck3d_out_dims',
           'ivx_neck3d_kitti_fwd', 'ivx_neck3d_nuscenes_fwd', 'ivx_neck3d_levels', 'ivx_neck3d_fast_fwd', 'ivx_neck3d_unet_fwd',
           'ivx_model_forward_levels', 'ivx_model_anchors', 'ivx_compute_projection', 'ivx_voxel_new_origin', 'ivx_fold_batchnorm',
           'ivx_model_trace', 'ivx_model_trace_count', 'ivx_model_trace_read',
           'ivx_model_detect_workspace_bytes', 'ivx_model_max_detections', 'ivx_model_detect', 'ivx_layout_head_decode', 'ivx_layout_extrinsics',
           'ivx_indoor_tail_workspace_bytes', 'ivx_indoor_tail_get_bboxes',
           'ivx_rescale_size', 'ivx_image_prep_u8', 'ivx_image_prep_lens_u8', 'ivx_map_prep_lens', 'ivx_image_prep_fmt_u8', 'ivx_yuv_matrix',
           'ivx_kitti_image_box_overlap', 'ivx_kitti_compute_statistics', 'ivx_kitti_collect_scores', 'ivx_kitti_fused_statistics']


def lib():
    """Load (once) and return the library.  Raises IvxError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IvxError(f'{LIB_PATH} is missing: build it with `python -m imvoxelnet_amd._build` '
                       '(or __graft_entry__.build()).  There is no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.ivx_version.restype = C.c_int
    L.ivx_last_error.restype = C.c_char_p
    L.ivx_conv_out_dims.argtypes = [C.POINTER(ConvDesc), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    for name in ('ivx_conv_fwd', 'ivx_conv_fwd_naive'):
        getattr(L, name).argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]
    L.ivx_conv_set_tile_override.argtypes = [C.c_int]
    L.ivx_conv_set_halo_mode.argtypes = [C.c_int]
    L.ivx_conv_set_epilogue_mode.argtypes = [C.c_int]
    L.ivx_conv_set_plan_mode.argtypes = [C.c_int]
    L.ivx_conv_winograd_output_blocks.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_output_blocks.restype = i32
    L.ivx_conv_winograd_output_amax.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, vp, vp, vp, i64, vp, vp]
    L.ivx_conv_winograd_input_amax.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, i64, vp, i32, vp]
    L.ivx_conv_winograd_fused_supported.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_fused_blocks.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_fused_blocks.restype = i32
    L.ivx_conv_winograd_gemm_output_amax.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.ivx_conv_winograd_bg_supported.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_bg_bytes.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_bg_bytes.restype = i64
    L.ivx_conv_winograd_bg_layer_offset.argtypes = [C.POINTER(ConvDesc), i32]
    L.ivx_conv_winograd_bg_layer_offset.restype = i64
    L.ivx_conv_winograd_bg_plan.argtypes = [C.POINTER(ConvDesc), vp, i32, C.POINTER(i32), vp, i64, vp]
    L.ivx_conv_winograd_input_bg.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, i64, vp, i32, vp, vp]
    L.ivx_conv_winograd_gemm_bg.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, i64, vp, vp]
    L.ivx_conv_winograd_output_bg.argtypes = [C.POINTER(ConvDesc), i32, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    L.ivx_bf16_pair_split.argtypes = [vp, i64, vp, vp]
    L.ivx_f16_pair_split.argtypes = [vp, i64, f32, vp, vp]
    L.ivx_conv_pair_supported.argtypes = [C.POINTER(ConvDesc)]
    L.ivx_bf16_pair_pack_filters.argtypes = [vp, i32, i32, i32, i32, vp]
    L.ivx_conv_route.argtypes = [C.POINTER(ConvDesc), i32, C.POINTER(ConvRouteOpts), C.POINTER(ConvRoute)]
    L.ivx_conv_pio_workspace_bytes.argtypes = [C.POINTER(ConvDesc), C.POINTER(PairIO)]
    L.ivx_conv_plan_query.argtypes = [C.POINTER(ConvDesc), C.POINTER(PairIO), C.c_int, C.c_int, C.POINTER(ConvPlanRec)]
    L.ivx_conv_tile_info.argtypes = [C.c_int, C.POINTER(i32)]
    L.ivx_conv_pio_workspace_bytes.restype = i64
    L.ivx_amax_f32.argtypes = [vp, i64, vp, vp]
    L.ivx_stem_pool_filter_bytes.restype = i64
    L.ivx_stem_pool_filter_bytes.argtypes = []
    L.ivx_stem_pool_pack_filters.argtypes = [vp, vp, vp, vp]
    L.ivx_stem_pool_out_dims.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ivx_stem_pool_fwd_pair.argtypes = [vp, i32, i32, i32, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp]
    L.ivx_bottleneck_supported.argtypes = [C.POINTER(BottleneckDesc)]
    L.ivx_bottleneck_fwd_pio.argtypes = [C.POINTER(BottleneckDesc), C.POINTER(BottleneckIO)] + [vp] * 12
    L.ivx_bottleneck_proj_supported.argtypes = [C.POINTER(BottleneckDesc), i32]
    L.ivx_bottleneck_proj_pack.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]
    L.ivx_bottleneck_proj_fwd_pio.argtypes = [C.POINTER(BottleneckDesc), i32, C.POINTER(BottleneckIO), f32] + [vp] * 12
    L.ivx_conv_fwd_pio.argtypes = [C.POINTER(ConvDesc), C.POINTER(PairIO), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.ivx_conv_fwd_pio_naive.argtypes = [C.POINTER(ConvDesc), C.POINTER(PairIO), vp, vp, vp, vp, vp, vp, vp]
    L.ivx_pair_pack_filters.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, C.POINTER(f32), C.POINTER(f32)]
    L.ivx_nchw_to_nhwc_amax.argtypes = [vp, i32, i32, i64, i32, vp, vp, vp]
    L.ivx_maxpool2d_fwd_pair.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]
    L.ivx_f16_pair_merge.argtypes = [vp, i64, vp, vp, vp]
    L.ivx_conv_workspace_bytes.argtypes = [C.POINTER(ConvDesc)]
    L.ivx_conv_workspace_bytes.restype = i64
    L.ivx_conv_fwd_ws.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, i64, vp]
    D = C.POINTER(ConvDesc)
    L.ivx_conv_winograd_supported.argtypes = [D, i32]
    L.ivx_conv_winograd_issued_fraction.argtypes = [D]
    L.ivx_conv_winograd_issued_fraction.restype = C.c_float
    L.ivx_conv_winograd_weight_elems.argtypes = [D, i32]
    L.ivx_conv_winograd_weight_elems.restype = i64
    L.ivx_conv_winograd_weights.argtypes = [D, i32, vp, vp, vp]
    L.ivx_conv_winograd_workspace_bytes.argtypes = [D, i32]
    L.ivx_conv_winograd_workspace_bytes.restype = i64
    L.ivx_conv_winograd_input.argtypes = [D, i32, vp, vp, i64, vp]
    L.ivx_conv_winograd_gemm.argtypes = [D, i32, vp, vp, i64, vp]
    L.ivx_conv_winograd_output.argtypes = [D, i32, vp, vp, vp, vp, vp, i64, vp]
    L.ivx_conv_winograd_fwd.argtypes = [D, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.ivx_maxpool2d_fwd.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    L.ivx_global_avgpool_fwd.argtypes = [vp, i32, i64, i32, vp, vp]
    L.ivx_global_avgpool_fwd_bf16.argtypes = [vp, i32, i64, i32, vp, vp]
    L.ivx_upsample_trilinear2x_fwd.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    L.ivx_dcn_im2col_fwd.argtypes = [vp, vp] + [i32] * 10 + [vp, vp]
    L.ivx_dcn_im2col_fwd_bf16.argtypes = [vp, vp] + [i32] * 10 + [vp, vp]
    L.ivx_dcn_im2col_fwd_pair.argtypes = [vp, vp, vp] + [i32] * 10 + [vp, vp, vp, vp]
    L.ivx_nchw_to_nhwc.argtypes = [vp, i32, i32, i64, i32, vp, vp]
    L.ivx_nhwc_to_nchw.argtypes = [vp, i32, i64, i32, vp, vp]
    L.ivx_rescale_size.argtypes = [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ivx_image_prep_u8.argtypes = [C.POINTER(ImagePrepDesc), vp, i64, i32, vp, vp]
    L.ivx_backproject_mean_fwd.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(f32), i32, i32, i32,
                                           vp, vp, vp]
    L.ivx_backproject_sum_fwd.argtypes = L.ivx_backproject_mean_fwd.argtypes
    L.ivx_backproject_mean_fwd_bf16.argtypes = L.ivx_backproject_mean_fwd.argtypes
    L.ivx_upsample_trilinear2x_fwd_bf16.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    L.ivx_volume_normalize_fwd.argtypes = [vp, vp, i64, i32, vp, vp]
    L.ivx_backproject_accum_fwd.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(f32), i32, i32, i32, vp, vp, i32, vp, vp, vp]
    L.ivx_backproject_accum_fwd_bf16.argtypes = L.ivx_backproject_accum_fwd.argtypes
    L.ivx_volume_mean_fwd.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp]
    if hasattr(L, 'ivx_backproject_fwd_ex'):       # (0.4.4; an older build of the same ABI, IVX_LIB_PATH, still loads: ops then refuses the bilinear rule)
        L.ivx_backproject_fwd_ex.argtypes = [C.POINTER(BackprojectDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, 'ivx_backproject_gather_fwd'):   # (0.4.6; an older build still loads: ops.backproject_gather_mean and windowed scenes then refuse)
        L.ivx_backproject_gather_fwd.argtypes = [C.POINTER(BackprojectDesc), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, 'ivx_backproject_lists_fwd'):    # (0.4.7; an older build still loads: ops.backproject_lists_accum_ / _mean_, scene batches and ragged batches then refuse)
        L.ivx_backproject_lists_fwd.argtypes = [C.POINTER(BackprojectDesc), C.POINTER(LiftLists), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, 'ivx_backproject_weighted_fwd'):  # (0.4.8; an older build still loads: ops.backproject_weighted_accum_ / _mean_ / volume_wmean and fading scenes then refuse)
        L.ivx_backproject_weighted_fwd.argtypes = [C.POINTER(BackprojectDesc), C.POINTER(LiftLists), C.POINTER(LiftWeights), vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ivx_volume_wmean_fwd.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp]
    if hasattr(L, 'ivx_volume_scroll_fwd'):        # (0.4.9; an older build still loads: ops.volume_scroll_ and scrolling scenes then refuse)
        L.ivx_volume_scroll_fwd.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp, vp, vp]
    if hasattr(L, 'ivx_backproject_mapped_fwd'):   # (0.5.0; an older build still loads: ops.backproject_mapped_accum_ / _mean_ and the scenes' pixel maps then refuse)
        L.ivx_backproject_mapped_fwd.argtypes = [C.POINTER(BackprojectDesc), C.POINTER(LiftLists), C.POINTER(LiftWeights), C.POINTER(LiftMaps), vp, vp, vp, vp, vp, vp, vp,
                                                 vp, vp]
    if hasattr(L, 'ivx_view_coverage_fwd'):        # (0.5.1; an older build still loads: ops.view_coverage and the scenes' coverage() / min_novelty= then refuse)
        L.ivx_view_coverage_fwd.argtypes = [C.POINTER(BackprojectDesc), C.POINTER(LiftLists), C.POINTER(LiftMaps), vp, vp, vp, vp, i32, f32, vp, vp]
    if hasattr(L, 'ivx_image_prep_lens_u8'):       # (0.5.2; an older build still loads: ops.image_prep_lens_u8 / map_prep_lens and the scenes' lens= / depth_frames= then refuse)
        L.ivx_image_prep_lens_u8.argtypes = [C.POINTER(ImagePrepDesc), C.POINTER(Lens), vp, i64, i32, vp, vp]
        L.ivx_map_prep_lens.argtypes = [C.POINTER(ImagePrepDesc), C.POINTER(Lens), vp, i32, i64, i64, f32, i32, i32, vp, vp]
    if hasattr(L, 'ivx_image_prep_fmt_u8'):        # (0.5.3; an older build still loads: ops.image_prep_fmt_u8 and format= then refuse; data.FrameFormat computes its named matrices itself)
        L.ivx_image_prep_fmt_u8.argtypes = [C.POINTER(ImagePrepDesc), C.POINTER(FrameFormat), C.POINTER(Lens), vp, i64, i32, vp, vp]
        L.ivx_yuv_matrix.argtypes = [i32, i32, C.POINTER(FrameFormat)]
    if hasattr(L, 'ivx_volume_warp_fwd'):          # (0.5.4; an older build still loads: ops.volume_warp and the scenes' warp() then refuse)
        L.ivx_volume_warp_fwd.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), f32] + [i32] * 6 + [vp] * 7
    if hasattr(L, 'ivx_volume_merge_fwd'):         # (0.5.5; an older build still loads: ops.volume_merge_ and the scenes' merge() then refuse)
        L.ivx_volume_merge_fwd.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)] + [C.POINTER(f32)] * 5 + [f32] + [i32] * 6 + [vp] * 7
    if hasattr(L, 'ivx_volume_pack_fwd'):          # (0.5.6; an older build still loads: ops.volume_pack / volume_unpack_ and the scenes' snapshot() / restore then refuse)
        L.ivx_volume_pack_scratch_bytes.argtypes = [i32] * 4
        L.ivx_volume_pack_scratch_bytes.restype = i64
        L.ivx_volume_pack_fwd.argtypes = [i32, C.POINTER(i32)] + [i32] * 5 + [vp] * 3 + [i32, i32] + [vp] * 7
        L.ivx_volume_unpack_fwd.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), i32] + [vp] * 4 + [i32] * 6 + [vp] * 4
    if hasattr(L, 'ivx_volume_match_fwd'):         # (0.5.7; an older build still loads: ops.volume_match and the scenes' match() / register() then refuse)
        L.ivx_volume_match_scratch_bytes.argtypes = [i32] * 6
        L.ivx_volume_match_scratch_bytes.restype = i64
        L.ivx_volume_match_fwd.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)] + [C.POINTER(f32)] * 4 + [C.POINTER(i32)] + [i32] * 6 + [vp] * 9
    if hasattr(L, 'ivx_volume_align_fwd'):         # (0.5.8; an older build still loads: ops.volume_align and the scenes' refine() then refuse)
        L.ivx_volume_align_scratch_bytes.argtypes = [i32] * 6
        L.ivx_volume_align_scratch_bytes.restype = i64
        L.ivx_volume_align_fwd.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)] + [C.POINTER(f32)] * 5 + [C.POINTER(i32)] + [i32] * 6 + [vp] * 10
    L.ivx_anchor_head_workspace_bytes.argtypes = [C.POINTER(AnchorHeadDesc)]
    L.ivx_anchor_head_workspace_bytes.restype = i64
    L.ivx_anchor_head_get_bboxes.argtypes = [C.POINTER(AnchorHeadDesc), vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ivx_fcos_head_workspace_bytes.argtypes = [i32, i32, i32]
    L.ivx_fcos_head_workspace_bytes.restype = i64
    L.ivx_fcos_head_level_candidates.argtypes = [vp, vp, vp, vp, f32] + [i32] * 12 + [vp, i64, vp, vp, vp, vp]
    L.ivx_nms_workspace_bytes.argtypes = [i32]
    L.ivx_nms_workspace_bytes.restype = i64
    L.ivx_nms_bev.argtypes = [vp, i32, f32, i32, vp, i64, vp, vp, vp]
    L.ivx_boxes_overlap_bev.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    L.ivx_aligned_3d_nms.argtypes = [vp, vp, vp, i32, f32, vp, vp, vp]
    L.ivx_aligned_3d_nms_workspace_bytes.argtypes = [i32]
    L.ivx_aligned_3d_nms_workspace_bytes.restype = i64
    L.ivx_aligned_3d_nms_ws.argtypes = [vp, vp, vp, i32, f32, vp, i64, vp, vp, vp]
    L.ivx_multiclass_nms_workspace_bytes.argtypes = [i32, i32]
    L.ivx_multiclass_nms_workspace_bytes.restype = i64
    L.ivx_multiclass_nms_bev.argtypes = [vp, vp, i32, i32, i32, f32, f32, i32, i32, vp, i64, vp, vp, vp, vp]
    L.ivx_create.argtypes = [C.POINTER(ModelCfg), C.POINTER(vp)]
    L.ivx_destroy.argtypes = [vp]
    L.ivx_weights_load.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
    L.ivx_weights_finalize.argtypes = [vp, vp]
    L.ivx_model_workspace_bytes.argtypes = [vp, i32, i32, i32, i32]
    L.ivx_model_workspace_bytes.restype = i64
    L.ivx_model_forward.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.ivx_backbone_fpn_workspace_bytes.argtypes = [vp, i32, i32, i32]
    L.ivx_backbone_fpn_workspace_bytes.restype = i64
    L.ivx_backbone_fpn_fwd.argtypes = [vp, vp, i32, i32, i32, vp, vp, i64, vp]
    L.ivx_neck3d_workspace_bytes.argtypes = [vp, i32]
    L.ivx_neck3d_workspace_bytes.restype = i64
    L.ivx_neck3d_out_dims.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ivx_neck3d_kitti_fwd.argtypes = [vp, vp, i32, vp, vp, i64, vp]
    L.ivx_neck3d_nuscenes_fwd.argtypes = [vp, vp, i32, vp, vp, i64, vp]
    L.ivx_topk_set_mode.argtypes = [i32]
    L.ivx_image_s2d_bf16.argtypes = [vp, i32, i32, i32, vp, vp]
    L.ivx_neck3d_levels.argtypes = [vp, i32, vp]
    L.ivx_neck3d_fast_fwd.argtypes = [vp, vp, i32, vp, vp, i64, vp]
    L.ivx_neck3d_unet_fwd.argtypes = [vp, vp, i32, vp, vp, i64, vp]
    L.ivx_model_forward_levels.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.ivx_model_anchors.argtypes = [vp, i32, i32, vp, i64]
    L.ivx_compute_projection.argtypes = [vp, vp, i32, C.c_double, vp]
    L.ivx_voxel_new_origin.argtypes = [vp, vp, vp, vp]
    L.ivx_fold_batchnorm.argtypes = [vp, vp, vp, vp, vp, f32, i32, vp, vp]
    L.ivx_model_calibrate_fp8.argtypes = [vp, vp, i32, i32, i32, f32, vp, i64, vp]
    L.ivx_model_calibrate_fp8_ex.argtypes = [vp, vp, i32, i32, i32, f32, i32, i32, vp, i64, vp]
    L.ivx_amax_bf16.argtypes = [vp, i64, vp, vp]
    L.ivx_model_trace.argtypes = [vp, i32]
    L.ivx_model_detect_workspace_bytes.argtypes = [vp, i32, i32, i32, i32]
    L.ivx_model_detect_workspace_bytes.restype = i64
    L.ivx_model_max_detections.argtypes = [vp, i32, i32, i32, i32]
    L.ivx_model_max_detections.restype = i32
    L.ivx_model_detect.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ivx_layout_head_decode.argtypes = [vp, vp, vp, vp]
    L.ivx_layout_extrinsics.argtypes = [vp, vp]
    L.ivx_indoor_tail_workspace_bytes.argtypes = [vp]
    L.ivx_indoor_tail_workspace_bytes.restype = i64
    L.ivx_indoor_tail_get_bboxes.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.ivx_conv_winograd_set_variant.argtypes = [i32, i32]
    L.ivx_ubench_mfma.argtypes = [i32, vp, i64, C.POINTER(C.c_double), vp]
    L.ivx_ubench_copy.argtypes = [vp, vp, i64, C.POINTER(C.c_double), vp]
    L.ivx_model_trace_count.argtypes = [vp]
    L.ivx_model_trace_count.restype = i32
    L.ivx_model_trace_read.argtypes = [vp, i32, C.POINTER(TraceRec)]
    declare_plan_view(L)
    # ctypes' default restype (c_int) is the int status every other entry point returns; the 64-bit queries must have been
    # declared explicitly above (a missing one would silently truncate)
    wide = [n for n in EXPORTS if n.endswith(('_workspace_bytes', '_weight_elems')) and getattr(L, n).restype is not C.c_int64]
    assert not wide, f'int64-returning entry points without an explicit restype: {wide}'
    _lib = L
    return L


def check(rc, what=''):
    if rc != 0:
        msg = lib().ivx_last_error().decode('utf-8', 'replace')
        if rc == -1:
            raise ValueError(f'{what}: {msg}')
        raise IvxError(f'{what}: status {rc}: {msg}')
