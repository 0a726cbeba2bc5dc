# -*- coding: utf-8 -*-
"""ctypes binding of libyolov4_amd.so (include/yolov4_amd.h).

The library is the product: there is no Python / PyTorch fallback for any entry
point.  `lib()` raises if the shared object is missing; every call goes through
`check()` which raises `Y4Error` on a non-zero status.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('Y4_LIB_PATH') or os.path.join(_HERE, 'lib', 'libyolov4_amd.so')   # override: kernel experiments

ACT_IDS = {'linear': 0, 'leaky_relu': 1, 'mish': 2, 'relu': 3}


class Y4Error(RuntimeError):
    pass


P = c_void_p        # every device / host pointer
I, L, F, Z = c_int, c_longlong, c_float, c_size_t

# name -> (restype, argtypes); mirrors include/yolov4_amd.h one to one
PROTOTYPES = {
    'y4_strerror': (c_char_p, [I]),
    'y4_version': (I, []),
    'y4_device_count': (I, []),
    'y4_set_conv_mode': (I, [I]),
    'y4_get_conv_mode': (I, []),
    'y4_set_planes_bf16': (I, [I]),
    'y4_get_planes_bf16': (I, []),
    'y4_conv_planes_fit': (I, [I, I, I, I, I, I, I, I]),
    'y4_conv2d_fwd_workspace': (Z, [I, I, I]),
    'y4_conv2d_fwd_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, P, I, P, I, P, P, P, Z, P]),
    'y4_amax_f32': (I, [P, I, L, I, P, P]),
    'y4_conv2d_prepared_bytes': (Z, [I, I]),
    'y4_conv2d_prepare_filter_f32': (I, [P, I, I, P, Z, P]),
    'y4_conv2d_fwd_prepared_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, P, I, P, I, P, P, P]),
    'y4_amax_merge_u32': (I, [P, P, P]),
    'y4_last_conv_kernel': (I, [ctypes.c_char_p, I]),
    'y4_conv2d_bnstats_workspace': (Z, [I, I, I, I, I, I, I]),
    'y4_conv2d_fwd_bnstats_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, Z, P, P, P, Z, P, Z, P]),
    'y4_planes_split_f32': (I, [P, I, L, I, P, P, P]),
    'y4_planes_split_into_f32': (I, [P, I, L, I, P, P, I, I, P]),
    'y4_conv2d_fwd_planes_f32': (I, [P, P, P, I, I, I, I, I, I, I, I, P, Z, P, P, P, Z, P, Z, I, P, P]),
    'y4_conv2d_dgrad_planes_f32': (I, [P, P, P, I, I, I, I, I, I, I, I, P, Z, P, P, I, P]),
    'y4_conv2d_wgrad_planes_workspace': (Z, [I, I, I, I, I, I, I]),
    'y4_conv2d_wgrad_planes_f32': (I, [P, P, P, I, I, I, I, I, I, I, P, Z, P, P, P]),
    'y4_conv2d_generic_fwd_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, P, I, P, I, P]),
    'y4_conv2d_generic_dgrad_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, I, P]),
    'y4_conv2d_generic_wgrad_f32': (I, [P, I, P, I, P, I, I, I, I, I, I, I, P]),
    'y4_conv2d_stem_dgrad_f32': (I, [P, I, P, P, L, L, L, L, I, I, I, I, P]),
    'y4_conv2d_stem_fwd_f32': (I, [P, L, L, L, L, P, P, I, I, I, I, I, P, P, I, P, P]),
    'y4_conv2d_dgrad_workspace': (Z, [I, I, I]),
    'y4_conv2d_dgrad_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, I, P, Z, P, P, I, P]),
    'y4_conv2d_wgrad_workspace': (Z, [I, I, I, I, I, I, I]),
    'y4_conv2d_wgrad_f32': (I, [P, I, P, I, P, I, I, I, I, I, I, I, P, Z, P, P, P]),
    'y4_conv2d_stem_wgrad_workspace': (Z, [I, I, I, I]),
    'y4_conv2d_stem_wgrad_f32': (I, [P, L, L, L, L, P, I, P, I, I, I, I, P, Z, P]),
    'y4_stem_fused_ok': (I, [L, L, L, L, I, I, I, I]),
    'y4_stem_bn_act_fwd_workspace': (Z, [I, I, I, I]),
    'y4_stem_bn_act_fwd_f32': (I, [P, L, L, L, L, P, I, I, I, I, P, P, I, P, P, P, P, P, F, F, P, I, P, P, Z, P]),
    'y4_stem_bn_act_bwd_workspace': (Z, [I, I, I, I]),
    'y4_stem_bn_act_bwd_f32': (I, [P, L, L, L, L, P, P, I, P, P, P, P, I, I, I, I, I, P, P, P, P, Z, P]),
    'y4_bn_workspace': (Z, [L, I]),
    'y4_bn_finalize_workspace': (Z, [I]),
    'y4_bn_finalize_partials_f32': (I, [P, L, L, I, P, P, P, P, P, F, F, P, Z, P]),
    'y4_bn_stats_f32': (I, [P, I, L, I, P, P, P, P, P, F, F, P, Z, P]),
    'y4_bn_act_fwd_f32': (I, [P, I, P, P, P, P, I, P, I, P, I, L, I, P, I, P, P, P]),
    'y4_bn_planes_bound_f32': (I, [P, P, I, L, P, P, P]),
    'y4_bn_act_bwd_f32': (I, [P, I, P, I, P, P, P, P, I, P, I, P, P, L, I, P, Z, P, P, P, I, P]),
    'y4_conv1x1_bn_act_bwd_fused_workspace': (Z, [L, I, I]),
    'y4_conv1x1_bn_act_bwd_fused_f32': (I, [P, I, P, I, P, P, P, P, I, P, P, L, I, I, P, I, P, P, P, P, I, P, I, P, P, Z, P, I, P]),
    'y4_bias_grad_workspace': (Z, [L, I]),
    'y4_bias_grad_f32': (I, [P, I, L, I, P, P, Z, P]),
    'y4_bn_fold_f32': (I, [P, P, P, P, F, P, P, I, P]),
    'y4_copy_channels_f32': (I, [P, I, P, I, L, I, P]),
    'y4_add_f32': (I, [P, I, P, I, P, I, L, I, P]),
    'y4_maxpool_s1_fwd_f32': (I, [P, I, P, I, P, I, I, I, I, I, P]),
    'y4_maxpool_s1_bwd_f32': (I, [P, I, P, P, I, I, I, I, I, I, I, P]),
    'y4_maxpool2x2_s2_fwd_f32': (I, [P, I, P, I, P, I, I, I, I, P]),
    'y4_maxpool2x2_s2_bwd_f32': (I, [P, I, P, P, I, I, I, I, I, P]),
    'y4_fork_half_bwd_f32': (I, [P, I, P, I, P, I, L, I, P]),
    'y4_conv2d_stem_s2_fwd_f32': (I, [P, L, L, L, L, P, P, I, I, I, I, I, P, P, I, P]),
    'y4_conv2d_stem_s2_wgrad_workspace': (Z, [I, I, I, I]),
    'y4_conv2d_stem_s2_wgrad_f32': (I, [P, L, L, L, L, P, I, P, I, I, I, I, P, Z, P]),
    'y4_upsample2x_fwd_f32': (I, [P, I, P, I, I, I, I, I, P]),
    'y4_upsample2x_bwd_f32': (I, [P, I, P, I, I, I, I, I, P]),
    'y4_yolo_decode_train_f32': (I, [P, I, P, P, I, I, I, I, P, P]),
    'y4_yolo_decode_eval_f32': (I, [P, I, P, L, L, I, I, I, I, P, F, P]),
    'y4_yolo_decode_bwd_f32': (I, [P, I, P, P, P, I, I, I, I, P, P]),
    'y4_yolo_loss_workspace': (Z, [I, I, I, I, I]),
    'y4_yolo_loss_fwd_f32': (I, [P, P, P, I, I, I, I, I, F, F, P, I, P, P, P, P, Z, P]),
    'y4_yolo_loss_bwd_f32': (I, [P, I, P, P, P, I, I, I, I, I, P, Z, P]),
    'y4_yolo_loss_mask_output_f32': (I, [P, P, I, I, I, I, I, P, Z, P]),
    'y4_yolo_loss_dense_targets_f32': (I, [P, P, P, I, I, I, I, I, P, Z, P]),
    'y4_yolo_box_loss_fwd_f32': (I, [P, I, F, I, I, I, I, I, P, P, Z, P]),
    'y4_yolo_box_loss_bwd_f32': (I, [P, I, F, P, P, I, I, I, I, I, P, Z, P]),
    'y4_yolo_decode_train_ex_f32': (I, [P, I, P, P, I, I, I, I, P, F, P]),
    'y4_yolo_decode_eval_ex_f32': (I, [P, I, P, L, L, I, I, I, I, P, F, F, P]),
    'y4_yolo_decode_bwd_ex_f32': (I, [P, I, P, P, P, I, I, I, I, P, F, P]),
    'y4_yolo_decode_eval_rect_f32': (I, [P, I, P, L, L, I, I, I, I, I, P, F, F, P]),
    'y4_yolo_loss_workspace_ex': (Z, [I, I, I, I, I, F]),
    'y4_yolo_loss_fwd_ex_f32': (I, [P, P, P, I, I, I, I, I, F, F, P, I, P, F, F, P, P, P, Z, P]),
    'y4_yolo_loss_bwd_ex_f32': (I, [P, I, P, P, P, I, I, I, I, I, F, F, P, Z, P]),
    'y4_yolo_loss_mask_output_ex_f32': (I, [P, P, I, I, I, I, I, F, P, Z, P]),
    'y4_yolo_loss_dense_targets_ex_f32': (I, [P, P, P, I, I, I, I, I, F, F, P, Z, P]),
    'y4_yolo_box_loss_fwd_ex_f32': (I, [P, I, F, I, I, I, I, I, F, P, P, Z, P]),
    'y4_yolo_box_loss_bwd_ex_f32': (I, [P, I, F, P, P, I, I, I, I, I, F, F, P, Z, P]),
    'y4_yolo_loss_workspace_opts': (Z, [I, I, I, I, I, P]),
    'y4_yolo_loss_fwd_opts_f32': (I, [P, P, P, I, I, I, I, I, F, F, P, I, P, P, P, P, P, Z, P]),
    'y4_yolo_loss_bwd_opts_f32': (I, [P, I, P, P, P, I, I, I, I, I, P, P, Z, P]),
    'y4_yolo_loss_dense_targets_opts_f32': (I, [P, P, P, I, I, I, I, I, P, P, Z, P]),
    'y4_yolo_loss_stats_scratch': (Z, [I, I, I]),
    'y4_yolo_loss_stats_f64': (I, [P, P, P, I, I, I, I, I, P, P, Z, P, Z, P, P]),
    'y4_post_count_f32': (I, [P, I, L, I, F, I, P, P]),
    'y4_post_scan_i32': (I, [P, I, L, P, P, P]),
    'y4_post_compact_f32': (I, [P, P, P, I, I, P, P, P, P]),
    'y4_post_nms_workspace': (Z, [L, I]),
    'y4_post_nms_f32': (I, [P, I, L, I, F, F, P, L, P, P, P, Z, P]),
    'y4_post_count_ex_f32': (I, [P, I, L, I, F, I, I, P, P]),
    'y4_post_nms_ex_workspace': (Z, [L, I, P]),
    'y4_post_nms_ex_f32': (I, [P, I, L, I, F, F, P, P, L, P, P, P, Z, P]),
    'y4_post_topk_workspace': (Z, [L, I]),
    'y4_post_topk_compact_f32': (I, [P, P, P, I, I, I, L, P, P, P, P, Z, P]),
    'y4_post_wbf_workspace': (Z, [L, I]),
    'y4_post_wbf_f32': (I, [P, I, L, I, F, F, I, I, P, L, P, P, P, Z, P]),
    'y4_nms_workspace': (Z, [L]),
    'y4_nms_f32': (I, [P, P, L, F, I, P, P, P, Z, P]),
    'y4_bboxes_iou_f32': (I, [P, L, P, L, I, P, P]),
    'y4_act_fwd_f32': (I, [P, P, L, I, P]),
    'y4_act_bwd_f32': (I, [P, P, P, L, I, P]),
    'y4_upsample_nearest_fwd_f32': (I, [P, I, P, I, I, I, I, I, I, I, I, P]),
    'y4_upsample_nearest_bwd_f32': (I, [P, I, P, I, I, I, I, I, I, I, I, P]),
    'y4_adam_step_f32': (I, [P, P, P, P, L, F, F, F, F, F, I, F, P]),
    'y4_adam_hyper_f32': (I, [F, F, F, F, I, P]),
    'y4_adam_multi_step_f32': (I, [P, I, P, I, F, F, F, F, P]),
    'y4_sgd_multi_step_f32': (I, [P, I, P, I, F, P]),
    'y4_grad_sumsq_multi_f32': (I, [P, I, F, P, P]),
    'y4_grad_guard_f32': (I, [P, I, c_double, P, P]),
    'y4_adam_multi_step_guarded_f32': (I, [P, I, P, I, F, F, F, F, P, P]),
    'y4_sgd_multi_step_guarded_f32': (I, [P, I, P, I, F, P, P]),
    'y4_ema_multi_f32': (I, [P, I, F, P, P]),
    'y4_preprocess_u8_f32': (I, [P, I, I, L, I, P, L, L, L, I, P]),
    'y4_letterbox_batch_u8_f32': (I, [P, P, I, P, L, L, L, L, I, I, I, P]),
    'y4_augment_means_u8': (I, [P, P, I, P, P]),
    'y4_augment_mosaic_u8_f32': (I, [P, P, I, P, P, I, P, P, L, L, L, L, I, P]),
    'y4_avgpool_global_fwd_f32': (I, [P, I, P, I, I, I, I, P]),
    'y4_avgpool_global_bwd_f32': (I, [P, I, P, I, I, I, I, P]),
    'y4_linear_fwd_f32': (I, [P, I, P, P, P, I, I, I, I, P]),
    'y4_linear_bwd_f32': (I, [P, I, P, P, I, P, I, P, P, I, I, I, P]),
    'y4_ce_smooth_fwd_f32': (I, [P, I, P, I, I, c_double, P, P, P]),
    'y4_ce_smooth_bwd_f32': (I, [P, I, P, P, P, P, I, I, I, c_double, P]),
    'y4_topk_correct_f32': (I, [P, I, P, I, I, P, I, P, P, P]),
    'y4_coco_workspace': (Z, [I, I]),
    'y4_coco_match_f64': (I, [P, P, P, I, P, P, P, P, P, I, I, P, P, P, P, P, Z, P]),
    'y4_coco_accumulate_f64': (I, [P, P, P, I, P, P, P, I, P, P, P, P, P]),
    'y4_jpeg_parse_host': (I, [P, Z, P]),
    'y4_jpeg_entropy_host': (I, [P, Z, P, P, L, P]),
    'y4_jpeg_workspace': (Z, [P, I]),
    'y4_jpeg_decode_u8': (I, [P, P, I, P, Z, P]),
    'y4_jpeg_encode_setup': (I, [I, I, I, I, I, I, P, P]),
    'y4_jpeg_encode_u8': (I, [P, P, I, P]),
    'y4_jpeg_encode_bound': (Z, [P]),
    'y4_jpeg_encode_host': (I, [P, P, P, P, Z, P]),
    'y4_draw_boxes_u8': (I, [P, P, I, P]),
    'y4_rcrop_workspace': (Z, [P, I, I]),
    'y4_rcrop_coeffs_i32': (I, [P, P, I, I, P, Z, P]),
    'y4_rcrop_u8_f32': (I, [P, P, I, I, P, P, P, L, L, L, L, P, Z, P]),
    'y4_randaug_workspace': (Z, [I, I, I]),
    'y4_rcrop_randaug_u8_f32': (I, [P, P, I, I, P, P, P, L, L, L, L, P, Z, P, P, I, P, Z, P]),
    'y4_anchor_assign_f32': (I, [P, I, P, I, F, P, P, P, P]),
    'y4_anchor_fitness_f32': (I, [P, I, P, I, I, F, P, P]),
    'y4_tta_view_f32': (I, [P, I, I, I, I, L, L, L, L, P, I, I, L, L, L, L, I, I, F, F, I, F, P]),
    'y4_tta_merge_f32': (I, [P, I, L, I, P, L, L, F, I, F, F, P]),
}

ERR_FORMAT, ERR_UNSUPPORTED = 6, 7


NMS_METRICS = {'iou': 0, 'diou': 1}
NMS_SOFT = {None: 0, 'linear': 1, 'gaussian': 2}


class NmsOpts(ctypes.Structure):
    """y4_nms_opts (32 bytes)"""
    _fields_ = [('metric', c_int), ('soft', c_int), ('sigma', c_float), ('agnostic', c_int), ('max_det', c_int),
                ('reserved', c_int * 3)]


FOCAL_TERMS = {'obj': 1, 'cls': 2, 'obj+cls': 3}


class LossOpts(ctypes.Structure):
    """y4_loss_opts (36 bytes)"""
    _fields_ = [('iou_thresh', c_float), ('label_smooth', c_float), ('focal_gamma', c_float), ('focal_alpha', c_float),
                ('focal_terms', c_int), ('obj_iou_ratio', c_float), ('obj_iou_kind', c_int), ('obj_gain', c_float),
                ('cls_gain', c_float)]


class AugSrc(ctypes.Structure):
    """y4_aug_src (72 bytes)"""
    _fields_ = [('src', c_void_p), ('h', c_int), ('w', c_int), ('pitch', c_longlong), ('swap_rb', c_int),
                ('crop_left', c_int), ('crop_top', c_int), ('crop_w', c_int), ('crop_h', c_int), ('flip', c_int),
                ('color', c_int), ('dhue', c_float), ('dsat', c_float), ('dexp', c_float), ('win_x', c_int),
                ('win_y', c_int)]


class LetterboxSrc(ctypes.Structure):
    """y4_letterbox_src (48 bytes)"""
    _fields_ = [('src', c_void_p), ('h', c_int), ('w', c_int), ('pitch', c_longlong), ('swap_rb', c_int), ('nh', c_int),
                ('nw', c_int), ('top', c_int), ('left', c_int), ('reserved', c_int)]


class AugSample(ctypes.Structure):
    """y4_aug_sample (16 bytes)"""
    _fields_ = [('cut_x', c_int), ('cut_y', c_int), ('n_src', c_int), ('first', c_int)]


class JpegInfo(ctypes.Structure):
    """y4_jpeg_info (88 bytes)"""
    _fields_ = [('width', c_int), ('height', c_int), ('ncomp', c_int), ('hs', c_int * 3), ('vs', c_int * 3),
                ('mcus_x', c_int), ('mcus_y', c_int), ('blocks_w', c_int * 3), ('blocks_h', c_int * 3),
                ('restart_interval', c_int), ('orientation', c_int), ('reserved', c_int), ('coef_count', c_longlong)]


class JpegJob(ctypes.Structure):
    """y4_jpeg_job (512 bytes)"""
    _fields_ = [('coef', c_void_p), ('out', c_void_p), ('out_pitch', c_longlong), ('ws_offset', c_longlong),
                ('info', JpegInfo), ('apply_orientation', c_int), ('swap_rb', c_int), ('qt', (ctypes.c_uint16 * 64) * 3)]


class JpegEncJob(ctypes.Structure):
    """y4_jpeg_enc_job (512 bytes)"""
    _fields_ = [('pixels', c_void_p), ('coef', c_void_p), ('pitch', c_longlong), ('info', JpegInfo), ('swap_rb', c_int),
                ('reserved', c_int * 3), ('qt', (ctypes.c_uint16 * 64) * 3)]


class DrawBox(ctypes.Structure):
    """y4_draw_box (64 bytes)"""
    _fields_ = [('x1', c_int), ('y1', c_int), ('x2', c_int), ('y2', c_int), ('half', c_int), ('px1', c_int), ('py1', c_int),
                ('px2', c_int), ('py2', c_int), ('tx', c_int), ('ty', c_int), ('scale', c_int), ('text_off', c_int),
                ('text_len', c_int), ('color', ctypes.c_uint8 * 4), ('reserved', c_int)]


class DrawJob(ctypes.Structure):
    """y4_draw_job (72 bytes)"""
    _fields_ = [('image', c_void_p), ('pitch', c_longlong), ('width', c_int), ('height', c_int), ('boxes', c_void_p),
                ('boxes_host', c_void_p), ('text', c_void_p), ('glyphs', c_void_p), ('n_boxes', c_int), ('text_bytes', c_int),
                ('n_glyphs', c_int), ('reserved', c_int)]


class RcropJob(ctypes.Structure):
    """y4_rcrop_job (96 bytes)"""
    _fields_ = [('src', c_void_p), ('src_pitch', c_longlong), ('src_h', c_int), ('src_w', c_int), ('swap_rb', c_int),
                ('crop_x', c_int), ('crop_y', c_int), ('crop_w', c_int), ('crop_h', c_int), ('res_w', c_int), ('res_h', c_int),
                ('win_x', c_int), ('win_y', c_int), ('flip', c_int), ('paste_from', c_int), ('paste_x0', c_int),
                ('paste_y0', c_int), ('paste_x1', c_int), ('paste_y1', c_int), ('ws_offset', c_longlong)]


class RandaugOp(ctypes.Structure):
    """y4_randaug_op (40 bytes)"""
    _fields_ = [('op', c_int), ('a', c_int * 6), ('factor', c_float), ('bits', c_int), ('threshold', c_int)]


_lib = None


def lib():
    """The loaded library.  Fails loudly when it has not been built
    (python __graft_entry__.py / make -C yolov4_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise Y4Error(f'{LIB_PATH} is missing: build it with `make -C yolov4_amd/csrc` '
                          '(hipcc --offload-arch=gfx950); there is no fallback path')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
        if os.environ.get('Y4_CONV_MODE'):
            handle.y4_set_conv_mode(int(os.environ['Y4_CONV_MODE']))
    return _lib


def check(code, what=''):
    if code != 0:
        msg = lib().y4_strerror(code).decode()
        raise Y4Error(f'{what}: {msg} (code {code})')


def float_array(values):
    arr = (c_float * len(values))(*[float(v) for v in values])
    return arr


def int_array(values):
    return (c_int * len(values))(*[int(v) for v in values])
