"""ctypes binding of libicamd.so (include/icamd.h) -- the only way the package reaches the GPU kernels.

There is no CPU or PyTorch fallback: if the shared library is missing or a symbol is absent, import of the
compute path raises.  PyTorch is used for device memory (tensors), streams and torch.distributed only.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libicamd.so")

ABI_VERSION = 6
ERRORS = {1: "ICAMD_ERR_BAD_ARG", 2: "ICAMD_ERR_UNSUPPORTED", 3: "ICAMD_ERR_WORKSPACE", 4: "ICAMD_ERR_LAUNCH"}


class IcamdError(RuntimeError):
    pass


class BnBwdFuse(Structure):
    _fields_ = [("y", c_void_p), ("mask_src", c_void_p), ("mean", c_void_p), ("invstd", c_void_p), ("scale", c_void_p),
                ("shift", c_void_p), ("partials", c_void_p), ("relu", c_int)]


class ImageDesc(Structure):
    """include/icamd.h icamd_image_desc (88 bytes)."""
    _fields_ = [("src_offset", ctypes.c_int64), ("src_h", c_int), ("src_w", c_int), ("crop_top", c_int), ("crop_left", c_int),
                ("crop_h", c_int), ("crop_w", c_int), ("hflip", c_int), ("vflip", c_int), ("jitter_order", c_int * 3),
                ("jitter_factor", c_float * 3), ("erase_top", c_int), ("erase_left", c_int), ("erase_h", c_int),
                ("erase_w", c_int), ("erase_seed", ctypes.c_uint32), ("reserved", c_int)]


class AugOp(Structure):
    """include/icamd.h icamd_aug_op (64 bytes): one RandAugment op of one image (kind AUG_KINDS[name], 0 = identity)."""
    _fields_ = [("kind", c_int), ("arg", c_int), ("factor", c_float), ("fill", ctypes.c_uint8 * 3),
                ("reserved", ctypes.c_uint8), ("affine", c_double * 6)]


AUG_OP_BYTES = 64
AUG_KINDS = {"identity": 0, "affine": 1, "autocontrast": 2, "equalize": 3, "invert": 4, "posterize": 5, "solarize": 6,
             "solarize_add": 7, "color": 8, "contrast": 9, "brightness": 10, "sharpness": 11}


class ConvDesc(Structure):
    _fields_ = [(n, c_int) for n in ("N", "IH", "IW", "Cin", "OH", "OW", "Cout", "KH", "KW", "stride", "pad")]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


def conv_desc(N, IH, IW, Cin, Cout, KH, KW, stride, pad):
    OH = (IH + 2 * pad - KH) // stride + 1
    OW = (IW + 2 * pad - KW) // stride + 1
    return ConvDesc(N, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad)


# name -> (restype, argtypes); with _SIGNATURES_ADDED below it mirrors include/icamd.h one to one
_P = c_void_p
_SIGNATURES = {
    "icamd_abi_version": (c_int, []),
    "icamd_conv2d_fwd_gelu": (c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "icamd_conv2d_dgrad_gelu": (c_int, [_P, _P, _P, _P, _P, _P]),
    "icamd_conv2d_fwd_act": (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P]),
    "icamd_bn_fold_filters": (c_int, [_P, _P, _P, _P, _P, c_float, c_int, c_int, _P, _P, _P]),
    "icamd_conv2d_stats_rows": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv2d_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P]),
    "icamd_conv2d_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P]),
    "icamd_conv2d_dgrad_sub2": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "icamd_conv2d_dgrad_stats_rows": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv2d_dgrad_bnbwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, POINTER(BnBwdFuse), _P]),
    "icamd_conv2d_dgrad_bnred_supported": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv2d_dgrad_bnred": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P]),
    "icamd_bn_bwd_from_gy_partials": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P, c_size_t, _P]),
    "icamd_bn_apply_conv1x1_fused_supported": (c_int, [POINTER(ConvDesc)]),
    "icamd_bn_apply_conv1x1_fused": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "icamd_conv1x1_bn_bwd_fused_supported": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv1x1_bn_bwd_fused_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "icamd_conv1x1_bn_bwd_fused": (c_int, [POINTER(ConvDesc), _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t,
                                           _P, c_size_t, _P]),
    "icamd_conv2d_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "icamd_conv2d_wgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int, _P, c_size_t, _P]),
    "icamd_conv2d_wgrad_bias": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    # grouped 3x3 convolution (csrc/conv_grouped.hip): the dense descriptor plus the group count; filter [C][3][3][C/groups]
    "icamd_gconv3x3_supported": (c_int, [POINTER(ConvDesc), c_int]),
    "icamd_gconv3x3_fwd": (c_int, [POINTER(ConvDesc), c_int, _P, _P, _P, _P, _P]),
    "icamd_gconv3x3_fwd_act": (c_int, [POINTER(ConvDesc), c_int, _P, _P, _P, _P, c_int, _P]),
    "icamd_gconv3x3_dgrad": (c_int, [POINTER(ConvDesc), c_int, _P, _P, _P, _P]),
    "icamd_gconv3x3_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc), c_int]),
    "icamd_gconv3x3_wgrad": (c_int, [POINTER(ConvDesc), c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    # ResNet-D (csrc/conv_stem_deep.hip): 2x2 average pool of the shortcut, thin 3x3 convolutions (Cin 32) of the deep stem
    "icamd_avgpool2x2_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_avgpool2x2_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_conv3x3_thin_supported": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv3x3_thin_stats_rows": (c_int, [POINTER(ConvDesc)]),
    "icamd_conv3x3_thin_fwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, c_int, _P]),
    "icamd_conv3x3_thin_dgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P]),
    "icamd_conv3x3_thin_wgrad_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "icamd_conv3x3_thin_wgrad": (c_int, [POINTER(ConvDesc), _P, _P, _P, c_int, _P, c_size_t, _P]),
    "icamd_filter_transpose": (c_int, [_P, _P, _P, _P, c_int, _P]),
    "icamd_filter_transpose_tiled": (c_int, [_P, _P, _P, _P, c_int, _P]),
    "icamd_bn_workspace_bytes": (c_size_t, [c_int]),
    "icamd_bn_train_finalize": (c_int, [_P, c_int, c_int, c_double, _P, _P, _P, _P, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "icamd_bn_eval_coeffs": (c_int, [c_int, _P, _P, _P, _P, c_float, _P, _P, _P]),
    "icamd_bn_apply": (c_int, [_P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P]),
    "icamd_bn_apply_res_bn": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P]),
    "icamd_bn_bwd_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "icamd_bn_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_bn_bwd_maxpool3x3s2": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_bn_bwd_dual": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int,
                                  _P, _P, c_size_t, _P]),
    "icamd_bn_bwd_apply_workspace_bytes": (c_size_t, [c_int]),
    "icamd_bn_bwd_from_partials": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P, c_size_t, _P]),
    # squeeze-and-excitation tail of a bottleneck block (csrc/se_ops.hip)
    "icamd_se_squeeze_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "icamd_se_squeeze": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_se_excite_fwd": (c_int, [_P, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "icamd_se_bn_apply": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_se_bn_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "icamd_se_bn_bwd": (c_int, [_P] * 20 + [c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_layernorm_fwd": (c_int, [_P, _P, _P, _P, _P, _P, c_longlong, c_int, c_float, _P]),
    "icamd_layernorm_bwd_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "icamd_layernorm_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P, c_size_t, _P]),
    "icamd_gelu_fwd": (c_int, [_P, _P, c_longlong, _P]),
    "icamd_gelu_bwd": (c_int, [_P, _P, _P, c_longlong, _P]),
    "icamd_colsum_rows_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "icamd_colsum_rows": (c_int, [_P, c_longlong, c_int, c_int, _P, c_int, _P, c_size_t, _P]),
    "icamd_dwconv7_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv7_dgrad": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv7_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "icamd_dwconv7_wgrad": (c_int, [_P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv7_wgrad_bias_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "icamd_dwconv7_wgrad_bias": (c_int, [_P, _P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, _P]),
    "icamd_layerscale_fwd": (c_int, [_P, _P, _P, _P, _P, c_longlong, c_int, c_longlong, _P]),
    "icamd_layerscale_bwd_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "icamd_layerscale_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_longlong, c_int, c_longlong, c_int, _P, c_size_t, _P]),
    "icamd_layerscale_fold": (c_int, [_P, _P, _P, _P, c_int, c_int, c_longlong, _P]),
    "icamd_rows_fix": (c_int, [_P, c_int, _P, _P, c_longlong, _P, c_longlong, _P]),
    "icamd_dropped_colsum": (c_int, [_P, _P, c_int, c_longlong, c_int, _P, _P]),
    "icamd_layerscale_param_grads": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_float, c_int, c_int, _P, _P, _P, c_int, _P]),
    "icamd_vit_tokens_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "icamd_batch_sum": (c_int, [_P, c_longlong, c_int, c_longlong, _P, c_int, _P]),
    "icamd_strided_rows_copy": (c_int, [_P, c_longlong, _P, c_longlong, c_longlong, c_longlong, _P]),
    "icamd_fill_zero": (c_int, [_P, c_size_t, _P]),
    # attention: any T >= 1, D = 64.  T <= 208 runs on the LDS-resident kernels (csrc/attention.hip), T > 208 on the tiled ones
    # (csrc/attention_long.hip); ICAMD_ATTN_LONG=2 forces the tiled route for every T, 0 disables it (see include/icamd.h)
    "icamd_attention_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "icamd_attention_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    # Swin (csrc/window_attention.hip): shifted-window attention over the natural token order (D = 32, 2 <= window <= 8 or window 12), the
    # relative-position table <-> bias gather / scatter, patch merging fused with its LayerNorm (4C <= 2048)
    "icamd_window_attention_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "icamd_window_attention_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, _P]),
    "icamd_window_attention_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_window_attention_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_int, c_float, _P]),
    "icamd_relpos_bias_gather": (c_int, [_P, _P, c_int, c_int, _P]),
    "icamd_relpos_bias_scatter": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "icamd_patch_merge_ln_fwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "icamd_patch_merge_ln_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "icamd_patch_merge_ln_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_maxpool3x3s2_fwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_bn_relu_maxpool3x3s2_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_maxpool3x3s2_bwd": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "icamd_avgpool_fwd": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "icamd_avgpool_bwd": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "icamd_pack_input": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, _P]),
    "icamd_pack_input_rgb4": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int, _P]),
    "icamd_stem7x7s2_stats_rows": (c_int, [c_int, c_int, c_int]),
    "icamd_stem7x7s2_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_stem7x7s2_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "icamd_stem7x7s2_wgrad": (c_int, [_P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, _P]),
    "icamd_image_pipeline_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_image_pipeline": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), _P,
                                     _P, c_size_t, _P]),
    "icamd_image_pipeline_u8": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "icamd_image_pipeline_aug_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_image_pipeline_aug": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float),
                                         POINTER(c_float), _P, _P, c_size_t, _P]),
    "icamd_softmax_xent": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_float, c_float, c_float, _P, _P, _P, _P]),
    "icamd_step_metrics": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "icamd_grad_norm_workspace_bytes": (c_size_t, []),
    "icamd_grad_norm": (c_int, [_P, c_longlong, c_float, c_float, _P, _P, _P]),
    "icamd_adamw_ema": (c_int, [_P, _P, _P, _P, _P, _P, c_longlong, c_float, c_float, c_float, c_float, c_float, c_int,
                                c_float, c_float, _P, _P, _P, c_int, _P]),
    "icamd_grad_guard": (c_int, [_P, c_longlong, _P, _P]),
    "icamd_optim_ema": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_longlong, c_float, c_float, c_float, c_float, c_float,
                                c_int, c_float, c_float, _P, _P, _P, c_int, _P]),
    "icamd_lerp": (c_int, [_P, _P, c_longlong, c_float, _P, _P]),
    "icamd_f32_to_bf16": (c_int, [_P, _P, c_longlong, _P]),
    "icamd_colsum": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P]),
    "icamd_rccl_available": (c_int, []),
    "icamd_rccl_version": (c_int, []),
    "icamd_rccl_unique_id": (c_int, [_P]),
    "icamd_rccl_comm_init": (c_int, [_P, c_int, c_int, POINTER(c_void_p)]),
    "icamd_rccl_comm_info": (c_int, [_P, POINTER(c_int), POINTER(c_int)]),
    "icamd_rccl_comm_destroy": (c_int, [_P]),
    "icamd_allreduce_bucket_launch": (c_int, [_P, _P, c_longlong, c_int, c_int, _P]),
    "icamd_broadcast_launch": (c_int, [_P, _P, c_longlong, c_int, c_int, _P]),
    "icamd_prof_enable": (c_int, [c_int]),
    "icamd_prof_classes": (c_int, []),
    "icamd_prof_collect": (c_int, [POINTER(c_double), POINTER(c_longlong), POINTER(c_double), POINTER(c_double), c_int]),
}

# Entries added after the host layer's answers were recorded (tests/golden/capi_answers.json pins what every entry of _SIGNATURES
# answers without a GPU, recorded from the library before the C-ABI layer was split into units; that record covers _SIGNATURES and
# stays as it is).  Same form, bound by load() like the others; the tests that arrive with an entry hold its host layer.
_SIGNATURES_ADDED = {
    # ConvNeXt V2 (csrc/grn.hip): global response normalisation over [N][rows_per_image][C], C % 32 == 0, 128 <= C <= 6144
    "icamd_grn_supported": (c_int, [c_int, c_longlong, c_int]),
    "icamd_grn_workspace_bytes": (c_size_t, [c_int, c_longlong, c_int]),
    "icamd_grn_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_longlong, c_int, c_float, _P, c_size_t, _P]),
    "icamd_grn_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_longlong, c_int, c_float, _P, c_size_t, _P]),
    # MobileNet class (csrc/dwconv3x3.hip): depthwise 3x3 pad 1 stride 1 / 2 over NHWC bf16 (C % 8 == 0), optionally forming
    # relu6(x * scale + shift) on load; BatchNorm + ReLU6 apply and backward
    "icamd_dwconv3_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv3_stats_rows": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv3_fwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv3_dgrad": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv3_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv3_wgrad": (c_int, [_P, _P, _P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_bn_apply_relu6": (c_int, [_P, _P, _P, _P, c_longlong, c_int, _P]),
    "icamd_bn_bwd_relu6_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "icamd_bn_bwd_relu6": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_longlong, c_int, c_int, _P, c_size_t, _P]),
    # EfficientNet class (csrc/dwconv5x5.hip): depthwise 5x5 pad 2 stride 1 / 2 over NHWC bf16 (C % 8 == 0, no on-load form);
    # BatchNorm + SiLU apply (optionally gated), per-sample sums and backward; the excitation of an MBConv block (SiLU inside)
    "icamd_dwconv5_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv5_stats_rows": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv5_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv5_dgrad": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_dwconv5_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "icamd_dwconv5_wgrad": (c_int, [_P, _P, _P, c_int, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
    "icamd_bn_apply_silu": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "icamd_bn_silu_squeeze_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "icamd_bn_silu_squeeze": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_se_excite_silu_fwd": (c_int, [_P, c_float, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "icamd_se_silu_bwd_reduce_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "icamd_se_silu_bwd_reduce": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, _P, c_size_t, _P]),
    "icamd_se_excite_silu_bwd": (c_int, [_P] * 11 + [c_int, c_int, c_int, c_float, c_int, _P]),
    "icamd_bn_bwd_silu_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "icamd_bn_bwd_silu": (c_int, [_P] * 11 + [c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES) + tuple(_SIGNATURES_ADDED)

_lib = None


def load():
    """Load libicamd.so and bind every symbol of include/icamd.h; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IcamdError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in {**_SIGNATURES, **_SIGNATURES_ADDED}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.icamd_abi_version() != ABI_VERSION:
        raise IcamdError("libicamd.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        raise IcamdError(f"{what} failed: {ERRORS.get(rc, rc)}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require_gpu():
    if not torch.cuda.is_available():
        raise IcamdError("the imageclassification_amd compute path needs an AMD GPU (gfx950); none is visible")


PROF_CLASSES = ("conv_fwd", "conv_dgrad", "conv_wgrad", "bn_finalize", "bn_apply", "bn_bwd", "pool", "pack", "loss",
                "optimizer", "misc", "attn_fwd", "attn_bwd", "ln_fwd", "ln_bwd", "elementwise", "dwconv", "conv_bn_bwd_fused", "bn_apply_conv_fused")


def prof_collect(work=False):
    """{class: (elapsed_ms, calls)} accumulated since the last call (HIP events on the launch stream); with work=True
    {class: (elapsed_ms, calls, algorithmic_bytes, algorithmic_flops)} (include/icamd.h: icamd_prof_collect)."""
    lib = load()
    n = lib.icamd_prof_classes()
    assert n == len(PROF_CLASSES), (n, len(PROF_CLASSES))
    ms = (c_double * n)()
    calls = (c_longlong * n)()
    nbytes = (c_double * n)()
    flops = (c_double * n)()
    check(lib.icamd_prof_collect(ms, calls, nbytes, flops, n), "prof_collect")
    if work:
        return {PROF_CLASSES[i]: (ms[i], calls[i], nbytes[i], flops[i]) for i in range(n)}
    return {PROF_CLASSES[i]: (ms[i], calls[i]) for i in range(n)}
