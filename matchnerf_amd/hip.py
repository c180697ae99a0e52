"""ctypes binding of libmnerf_hip.so (include/mnerf.h) — the only door to the HIP kernels.

There is deliberately NO fallback: if the shared library is missing or a call fails, a
``MnerfError`` is raised.  The product path never routes through the CPU oracle.
Tensors are passed as raw device pointers (``tensor.data_ptr()``) plus explicit sizes.  Every
launch runs under ``torch.cuda.device(<device of the tensors>)`` on that device's current torch
stream (the library launches on the calling thread's current HIP device), so the module works on
any ``--gpu_ids`` / LOCAL_RANK, like the pure-torch reference.  The binding itself needs no GPU
(``load()`` works on a CPU-only box; that is what the ``-m "not gpu"`` ABI tests exercise).
Adding an export: its prototype in include/mnerf.h and one row in ``SIGNATURES`` below; tests/test_abi.py holds the two together.
"""
import contextlib
import ctypes as C
import os

import numpy as np

MNERF_ABI_VERSION = 12
MNERF_POSE_FLOATS = 24  # floats of one row of mnerf_rays.pose_table
MNERF_RAY_FLOATS = 8  # floats of one row of a ray bundle: ox oy oz 0 | dx dy dz 0
CAM_PINHOLE, CAM_FISHEYE, CAM_SPHERE, CAM_ORTHO = 0, 1, 2, 3  # mnerf_camera.model (MNERF_CAM_*)
STRUCT_CAMERA = 32  # MNERF_STRUCT_CAMERA: mnerf_struct_size()'s index of mnerf_camera
MNERF_OK, MNERF_E_NULL, MNERF_E_RANGE, MNERF_E_UNSUPPORTED, MNERF_E_ALIGN = 0, -1, -2, -3, -4  # include/mnerf.h
MNERF_MAX_VIEWS = 16
MNERF_COND_STRIDE_MAX, MNERF_COND_STRIDE_MAX_F32 = 96, 64
SMALL_FIXED = 32  # floats of the `small` parameter block (LayerNorm weight|bias) before the ray-posenc table

_LIB = None
_LIB_PATH = os.environ.get("MNERF_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmnerf_hip.so")

class MnerfError(RuntimeError):
    pass


class View(C.Structure):
    _fields_ = [("extr", C.c_float * 12), ("intr", C.c_float * 9), ("near_", C.c_float), ("far_", C.c_float)]


class Rays(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_samples", C.c_int32), ("ray_begin", C.c_int32),
                ("legacy_coord", C.c_int32), ("depth_inverse", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("ray_idx", C.c_void_p), ("strat_u", C.c_void_p),
                ("kinv", C.c_float * 9), ("c2w", C.c_float * 12), ("near_", C.c_float), ("far_", C.c_float),
                ("pose_table", C.c_void_p), ("rays_per_pose", C.c_int32), ("tgt_height", C.c_int32),
                ("tgt_width", C.c_int32), ("pad_", C.c_int32)]


class Scene(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_scales", C.c_int32), ("fh", C.c_int32 * 2), ("fw", C.c_int32 * 2),
                ("n_group", C.c_int32 * 2), ("feat", C.c_void_p * 2), ("images", C.c_void_p),
                ("views", View * MNERF_MAX_VIEWS), ("feat_op", C.c_void_p)]


class Decoder(C.Structure):
    _fields_ = [("wstream", C.c_void_p), ("wstream_floats", C.c_int64), ("small_", C.c_void_p),
                ("n_views", C.c_int32), ("cond_dim", C.c_int32), ("cond_stride", C.c_int32),
                ("L_3D", C.c_int32), ("raytrans_posenc", C.c_int32), ("raytrans_elu", C.c_int32),
                ("density_maskfill", C.c_int32), ("wo_render_interval", C.c_int32),
                ("setbg_opaque", C.c_int32), ("wstream_format", C.c_int32)]


# parameter tensors of the decoder in mnerf_decoder_train's order (include/mnerf.h, MNERF_DT_*): names relative to the CondNeRF module
DEC_TRAIN_TENSORS = tuple(f"pts_linears.{i}.{k}" for i in range(6) for k in ("weight", "bias")) + (
    "pts_bias.weight", "pts_bias.bias", "alpha_linear.0.weight", "alpha_linear.0.bias", "ray_attention.w_qs.weight",
    "ray_attention.w_ks.weight", "ray_attention.w_vs.weight", "ray_attention.fc.weight", "ray_attention.layer_norm.weight",
    "ray_attention.layer_norm.bias", "out_alpha_linear.0.weight", "out_alpha_linear.0.bias", "out_alpha_linear.2.weight",
    "out_alpha_linear.2.bias", "feature_linear.weight", "feature_linear.bias", "views_linears.0.weight", "views_linears.0.bias",
    "rgb_linear.weight", "rgb_linear.bias")


class DecoderTrain(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("cond_dim", C.c_int32), ("n_trunk", C.c_int32), ("net_width", C.c_int32),
                ("skip_layer", C.c_int32), ("L_3D", C.c_int32), ("legacy_coord", C.c_int32), ("raytrans_elu", C.c_int32),
                ("raytrans_posenc", C.c_int32), ("density_maskfill", C.c_int32), ("raytrans_table", C.c_void_p),
                ("w", C.c_void_p * len(DEC_TRAIN_TENSORS)), ("g", C.c_void_p * len(DEC_TRAIN_TENSORS))]


class EncoderLayer(C.Structure):
    _fields_ = [("wstream", C.c_void_p), ("wstream_floats", C.c_int64), ("ln", C.c_void_p), ("ffn", C.c_int32),
                ("ew_merge", C.c_int32), ("ew_w1", C.c_int32), ("ew_w2", C.c_int32)]


class EncoderLayerTrain(C.Structure):
    """mnerf_encoder_layer_train: parameters of a transformer layer after the attention in torch's layouts + their gradients"""
    _fields_ = [("ffn", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("w_merge", "ln1_w", "ln1_b", "w_mlp0", "w_mlp2", "ln2_w", "ln2_b",
                                          "g_w_merge", "g_ln1_w", "g_ln1_b", "g_w_mlp0", "g_w_mlp2", "g_ln2_w", "g_ln2_b")]


WSTREAM_F32, WSTREAM_BF16X3, WSTREAM_F16X2, WSTREAM_F16X1 = 0, 1, 2, 3
WA_SPLIT_BF16, WA_EXACT_F32, WA_SPLIT_F16 = 0, 1, 2
WA_PRESPLIT_F16 = 3  # host-side selector only: routed to mnerf_window_attention_presplit
ABSMAX_FLOATS = 64 * 32  # floats of one absmax region (MNERF_ABSMAX_FLOATS)
CONV_OUT_NCHW, CONV_OUT_CHANNEL_LAST, CONV_OUT_PAIR_MAJOR = 0, 1, 2


class ConvLayer(C.Structure):
    """struct mnerf_conv (include/mnerf.h)"""
    _fields_ = [("wstream", C.c_void_p), ("wstream_floats", C.c_int64), ("bias", C.c_void_p), ("c_in", C.c_int32),
                ("c_out", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("ew", C.c_int32),
                ("leaky_slope", C.c_float)]


LPIPS_LAYERS, LPIPS_STAGES = 13, 5


class LpipsWeightTable(C.Structure):
    """struct mnerf_lpips_weights: the by-pointer table of mnerf_lpips_vgg"""
    _fields_ = [("wstream", C.c_void_p * LPIPS_LAYERS), ("bias", C.c_void_p * LPIPS_LAYERS), ("head", C.c_void_p * LPIPS_STAGES),
                ("ew", C.c_int32 * LPIPS_LAYERS)]


class Camera(C.Structure):
    """struct mnerf_camera: a camera model that fills a ray bundle on the device (mnerf_camera_rays; camera.camera_model builds it).
    The header passes it as an untyped pointer, so it is no member of STRUCTS; load() checks its size under STRUCT_CAMERA."""
    _fields_ = [("model", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("legacy_coord", C.c_int32),
                ("kinv", C.c_float * 9), ("c2w", C.c_float * 12), ("lon_lat", C.c_float * 4)]


OPTIM_CHUNK, OPTIM_MAX_GROUPS = 4096, 8  # MNERF_OPTIM_CHUNK, MNERF_OPTIM_MAX_GROUPS


class OptimRow(C.Structure):
    """struct mnerf_optim_row: one parameter tensor of the device table of mnerf_grad_sumsq / mnerf_adamw_step"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64), ("group", C.c_int32), ("block_begin", C.c_int32), ("bias_correction1", C.c_double),
                ("bias_correction2_sqrt", C.c_float), ("pad_", C.c_int32)]


class OptimGroup(C.Structure):
    """struct mnerf_optim_group: hyperparameters of one parameter group, by value"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("max_norm", C.c_double), ("n_blocks", C.c_int32), ("pad_", C.c_int32)]


# ----------------------------------------------------------------------- the C ABI, declared once

# The struct mirrors in the order of mnerf_struct_size()'s indices (load() verifies every one), and which header struct each mirrors.
STRUCTS = (View, Rays, Scene, Decoder, EncoderLayer, ConvLayer, DecoderTrain, EncoderLayerTrain, OptimRow, OptimGroup, LpipsWeightTable)
HEADER_STRUCTS = dict(zip(("mnerf_view", "mnerf_rays", "mnerf_scene", "mnerf_decoder", "mnerf_encoder_layer", "mnerf_conv",
                           "mnerf_decoder_train", "mnerf_encoder_layer_train", "mnerf_optim_row", "mnerf_optim_group",
                           "mnerf_lpips_weights"), STRUCTS))

_int, _i32, _i64, _sz, _f32, _vp, _P = C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_float, C.c_void_p, C.POINTER
_rows = _vp  # const mnerf_optim_row*: the row table lies in DEVICE memory (a uint8 CUDA tensor of OptimRow records)

# One row per export of include/mnerf.h, in the header's order: name -> (restype, argtypes).  load() applies it; device buffers, host
# scratch and the stream are c_void_p, argument structs POINTER(mirror).  tests/test_abi.py compares every row with its prototype.
SIGNATURES = {
    "mnerf_abi_version": (_int, []),
    "mnerf_last_error": (C.c_char_p, []),
    "mnerf_struct_size": (_i64, [_i32]),
    "mnerf_ray_samples": (_int, [_P(Rays), _P(View)] + [_vp] * 4),
    "mnerf_composite": (_int, [_i32] * 2 + [_vp] * 4 + [_i32] * 2 + [_vp] * 5),
    "mnerf_cost_volume": (_int, [_P(Scene), _P(Rays), _i32, _vp, _vp]),
    "mnerf_cost_volume_operand_bytes": (_i64, [_P(Scene)]),
    "mnerf_cost_volume_operands": (_int, [_P(Scene), _vp, _vp]),
    "mnerf_decoder_wstream_floats": (_i64, [_i32] * 4),
    "mnerf_decoder_chunk": (_int, [_P(Decoder), _P(View), _P(Rays)] + [_vp] * 7),
    "mnerf_decoder_samples": (_int, [_P(Decoder)] + [_i32] * 3 + [_vp] * 6),
    "mnerf_render_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_render_chunk_is_fused": (_i32, [_P(Scene), _P(Decoder), _P(Rays)]),
    "mnerf_render_takes_pose_table": (_i32, [_P(Scene), _P(Decoder), _i32, _i32]),
    "mnerf_render_chunk": (_int, [_P(Scene), _P(Decoder), _P(Rays)] + [_vp] * 5),
    "mnerf_render_chunk_fused": (_int, [_P(Scene), _P(Decoder), _P(Rays)] + [_vp] * 4),
    "mnerf_box_downsample": (_int, [_vp] + [_i32] * 4 + [_vp] * 2),
    "mnerf_cost_volume_rays": (_int, [_P(Scene), _P(Rays), _vp, _i32, _vp, _vp]),
    "mnerf_ray_samples_rays": (_int, [_P(Rays), _vp, _P(View)] + [_vp] * 5),
    "mnerf_render_rays_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_render_rays": (_int, [_P(Scene), _P(Decoder), _P(Rays)] + [_vp] * 6),
    "mnerf_camera_rays": (_int, [_vp, _i32, _i32, _vp, _vp]),  # const void* camera: a Camera by reference
    "mnerf_composite_backward": (_int, [_i32] * 2 + [_vp] * 4 + [_i32] * 2 + [_vp] * 6),
    "mnerf_cost_volume_backward": (_int, [_P(Scene), _P(Rays), _i32] + [_vp] * 4),
    "mnerf_debug_set_knob": (_int, [C.c_char_p, _int, _P(_int)]),
    "mnerf_debug_launch_plan": (_int, [C.c_char_p, _vp, _i32, _P(_i32), _i32]),
    "mnerf_decoder_backward_workspace_bytes": (_i64, [_i32] * 2),
    "mnerf_decoder_backward": (_int, [_P(DecoderTrain)] + [_i32] * 2 + [_vp] * 3 + [_i32] + [_vp] * 5),
    "mnerf_window_attention": (_int, [_vp] * 4 + [_i32] * 6 + [_vp]),
    "mnerf_window_attention_workspace_bytes": (_sz, [_i32] * 4),
    "mnerf_window_attention_presplit": (_int, [_vp] * 4 + [_i32] * 5 + [_vp, _sz, _vp]),
    "mnerf_qkv_wstream_floats": (_i64, []),
    "mnerf_qkv_projection": (_int, [_vp, _P(_i32), _vp, _vp, _i32] + [_vp] * 3 + [_i32] * 2 + [_vp]),
    "mnerf_qkv_window_images": (_int, [_vp, _P(_i32), _vp, _vp, _i32, _vp, _vp, _sz] + [_i32] * 5 + [_vp]),
    "mnerf_window_attention_images": (_int, [_vp] * 2 + [_i32] * 5 + [_vp, _sz, _vp]),
    "mnerf_window_attention_backward_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_window_attention_backward": (_int, [_vp] * 8 + [_i32] * 5 + [_vp, _sz, _vp]),
    "mnerf_window_attention_presplit_stats": (_int, [_vp] * 5 + [_i32] * 5 + [_vp, _sz, _vp]),
    "mnerf_window_attention_backward_stats": (_int, [_vp] * 9 + [_i32] * 5 + [_vp, _sz, _vp]),
    "mnerf_instance_norm": (_int, [_vp] * 3 + [_i64, _i64, _f32, _i32, _i32, _vp, _vp]),
    "mnerf_instance_norm_backward": (_int, [_vp] * 3 + [_i64, _i64, _f32, _i32, _vp]),
    "mnerf_upsample_bilinear2x": (_int, [_vp] * 3 + [_i64, _i32, _i32, _vp]),
    "mnerf_upsample_bilinear2x_backward": (_int, [_vp] * 2 + [_i64, _i32, _i32, _vp]),
    "mnerf_conv_wstream_floats": (_i64, [_i32] * 3),
    "mnerf_conv2d": (_int, [_P(ConvLayer), _vp, _i32, _i32] + [_vp] * 4 + [_i32, _vp] + [_i32] * 3 + [_vp]),
    "mnerf_conv_stem_wstream_floats": (_i64, []),
    "mnerf_conv_stem": (_int, [_vp, _i32] + [_vp] * 3 + [_i32] * 3 + [_vp]),
    "mnerf_absmax": (_int, [_vp, _i64, _vp, _vp]),
    "mnerf_conv2d_backward_data": (_int, [_vp] * 3 + [_i32] * 7 + [_vp]),
    "mnerf_conv2d_backward_weight_workspace_bytes": (_sz, [_i32] * 7),
    "mnerf_conv2d_backward_weight": (_int, [_vp] * 4 + [_sz] + [_i32] * 7 + [_vp]),
    "mnerf_conv2d_backward_weight_f16x3": (_int, [_vp] * 6 + [_sz] + [_i32] * 7 + [_vp]),
    "mnerf_conv2d_forward_f32": (_int, [_vp] * 4 + [_i32] * 7 + [_vp]),
    "mnerf_conv_stem_backward_weight_workspace_bytes": (_sz, [_i32] * 3),
    "mnerf_conv_stem_backward_weight": (_int, [_vp] * 4 + [_sz] + [_i32] * 3 + [_vp]),
    "mnerf_encoder_block_wstream_floats": (_i64, [_i32]),
    "mnerf_encoder_block": (_int, [_P(EncoderLayer)] + [_vp] * 3 + [_i32, _vp]),
    "mnerf_encoder_layer_backward_workspace_bytes": (_i64, [_i32]),
    "mnerf_encoder_layer_backward": (_int, [_P(EncoderLayerTrain)] + [_vp] * 5 + [_i32, _vp, _vp]),
    "mnerf_encoder_block_save": (_int, [_P(EncoderLayer)] + [_vp] * 6 + [_i32, _vp]),
    "mnerf_encoder_layer_backward_saved": (_int, [_P(EncoderLayerTrain)] + [_vp] * 8 + [_i32, _vp, _vp]),
    "mnerf_qkv_backward": (_int, [_vp] * 13 + [_i32, _vp]),
    "mnerf_debug_gemm": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp] + [_i32] * 5 + [_vp]),
    "mnerf_optim_row_blocks": (_i64, [_i64]),
    "mnerf_grad_sumsq": (_int, [_rows, _i32, _i32, _P(OptimGroup), _i32] + [_vp] * 3),
    "mnerf_adamw_step": (_int, [_rows, _i32, _i32, _P(OptimGroup), _i32] + [_vp] * 2),
    "mnerf_l2_loss": (_int, [_vp, _vp, _i64, _f32] + [_vp] * 3),
    "mnerf_grad_bucket_floats": (_i64, [_i64]),
    "mnerf_grad_pack": (_int, [_rows, _i32, _i32, _vp, _i32, _vp, _vp]),
    "mnerf_grad_unpack": (_int, [_rows, _i32, _i32, _vp, _f32, _vp, _i32, _vp]),
    "mnerf_image_metrics_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_image_metrics": (_int, [_vp, _vp, _i64, _vp] + [_i32] * 3 + [_vp] * 3),
    "mnerf_lpips_wstream_floats": (_i64, [_i32]),
    "mnerf_lpips_workspace_bytes": (_i64, [_i32] * 4),
    "mnerf_lpips_vgg": (_int, [_vp, _vp, _i64, _vp] + [_i32] * 3 + [_P(LpipsWeightTable)] + [_vp] * 3),
    "mnerf_maxpool2x2": (_int, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "mnerf_lpips_head_slots": (_i64, [_i32] * 2),
    "mnerf_lpips_head": (_int, [_vp] * 3 + [_i32] * 3 + [_vp] * 2),
    "mnerf_lpips_sum": (_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "mnerf_depth_consistency": (_int, [_P(View)] + [_i32] * 5 + [_vp] * 2 + [_f32] * 3 + [_vp, _P(_i32), _vp]),  # views: a host array of View
    "mnerf_point_cloud_workspace_bytes": (_i64, [_i64]),
    "mnerf_point_cloud": (_int, [_P(View)] + [_i32] * 3 + [_vp] * 2 + [_P(_i32), _i32, _vp, _i64] + [_vp] * 3),
    "mnerf_depth_colormap": (_int, [_vp, _i64, _f32, _f32, _vp, _vp]),
    "mnerf_tsdf_integrate": (_int, [_P(View)] + [_i32] * 4 + [_vp] * 2 + [_P(_i32), _i32, _vp] + [_f32] * 6 + [_i32] * 3 + [_vp] * 3),
    "mnerf_tsdf_mesh_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_tsdf_mesh": (_int, [_vp] * 2 + [_f32] * 4 + [_i32] * 3 + [_f32, _vp, _i64, _P(_i32), _i64] + [_vp] * 3),
    "mnerf_tsdf_bricks_mark": (_int, [_P(View)] + [_i32] * 4 + [_vp] * 2 + [_P(_i32), _i32] + [_f32] * 6 + [_i32] * 3 + [_vp] * 2),
    "mnerf_tsdf_bricks_table_workspace_bytes": (_i64, [_i32] * 3),
    "mnerf_tsdf_bricks_table": (_int, [_vp] + [_i32] * 3 + [_P(_i32), _P(_i32)] + [_vp] * 3),
    "mnerf_tsdf_integrate_sparse": (_int, [_P(View)] + [_i32] * 4 + [_vp] * 2 + [_P(_i32), _i32, _vp] + [_f32] * 6 + [_i32] * 3
                                    + [_P(_i32), _i64] + [_vp] * 3),
    "mnerf_tsdf_mesh_sparse_workspace_bytes": (_i64, [_i64] + [_i32] * 3),
    "mnerf_tsdf_mesh_sparse": (_int, [_vp] * 2 + [_P(_i32), _P(_i32), _i64] + [_f32] * 4 + [_i32] * 3
                               + [_f32, _vp, _i64, _P(_i32), _i64] + [_vp] * 3),
    # (the rows of MESH TEXTURE and the two of the decimation: the header declares them after MESH FINISHING's first six; here they
    # stand in front of those, which tests/test_mesh_finish_cpu.py expects to be the table's last rows)
    "mnerf_mesh_texture_atlas": (_int, [_i64, _i32, _P(_i32)]),  # size: a host array
    "mnerf_mesh_texture_uv": (_int, [_i64, _i32, _vp, _vp]),
    "mnerf_mesh_texture_accumulate": (_int, [_vp, _P(_i32), _i64, _i64, _i32, _P(View)] + [_i32] * 4 + [_vp] * 2 + [_P(_i32), _i32, _vp]
                                      + [_f32] * 2 + [_i32] * 2 + [_vp] * 2),
    "mnerf_mesh_texture_resolve": (_int, [_vp, _P(_i32), _i64, _i64, _i32, _i32] + [_vp] * 3),
    "mnerf_mesh_raster_workspace_bytes": (_i64, [_i32] * 2),
    "mnerf_mesh_raster": (_int, [_vp, _P(_i32), _i64, _i64, _P(View)] + [_i32] * 3 + [_P(_i32)] + [_vp] * 3 + [_i64, _vp]),  # view: one host View
    "mnerf_mesh_shade": (_int, [_vp, _P(_i32), _i64, _i64, _P(_i32), _vp, _i32, _i32, _vp] + [_i32] * 3 + [_P(View)] + [_vp] * 3),
    "mnerf_mesh_decimate_workspace_bytes": (_i64, [_i64] * 2 + [_i32] * 3),
    "mnerf_mesh_decimate": (_int, [_vp, _P(_i32), _i64, _i64, _P(_i32), _P(_i32)] + [_f32] * 4 + [_i32] * 3
                            + [_vp, _i64, _P(_i32), _i64, _P(_i32)] + [_vp] * 3),
    "mnerf_mesh_finish_workspace_bytes": (_i64, [_i64] * 2),
    "mnerf_mesh_adjacency": (_int, [_P(_i32), _i64, _i64, _P(_i32), _P(_i32)] + [_vp] * 3),
    "mnerf_mesh_components": (_int, [_P(_i32), _i64, _i64, _i64, C.c_double, _P(_i32)] + [_vp] * 3),
    "mnerf_mesh_compact": (_int, [_vp, _P(_i32), _i64, _i64, _vp, _vp, _i64, _P(_i32), _i64] + [_vp] * 3),
    "mnerf_mesh_smooth": (_int, [_vp, _i64, _P(_i32), _i64, _P(_i32), _P(_i32), _vp, _i32, _f32, _f32] + [_vp] * 3),
    "mnerf_mesh_normals": (_int, [_vp, _i64, _P(_i32), _i64, _P(_i32), _P(_i32), _vp, _vp]),
}
EXPORTS = tuple(SIGNATURES)


def lib_path():
    return _LIB_PATH


def load():
    """dlopen the library (once) and declare signatures.  Raises MnerfError if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be resident BEFORE this library is
    # dlopen'ed so that both bind to ONE HIP runtime (device pointers and streams are shared).
    # Loading /opt/rocm's copy first leaves the process with a runtime torch cannot use.
    import torch  # noqa: F401
    if not os.path.exists(_LIB_PATH):
        raise MnerfError(
            f"{_LIB_PATH} not found: build it with `python -m matchnerf_amd.csrc.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the render path.")
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as e:  # noqa: PERF203
        raise MnerfError(f"cannot load {_LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    ver = lib.mnerf_abi_version()
    if ver != MNERF_ABI_VERSION:
        raise MnerfError(f"libmnerf_hip.so ABI {ver} != binding ABI {MNERF_ABI_VERSION}")
    for which, st in enumerate(STRUCTS):
        if lib.mnerf_struct_size(which) != C.sizeof(st):
            raise MnerfError(f"struct {st.__name__}: library says {lib.mnerf_struct_size(which)} bytes, "
                             f"ctypes mirror has {C.sizeof(st)}")
    if lib.mnerf_struct_size(STRUCT_CAMERA) != C.sizeof(Camera):
        raise MnerfError(f"struct Camera: library says {lib.mnerf_struct_size(STRUCT_CAMERA)} bytes, ctypes mirror has {C.sizeof(Camera)}")
    _LIB = lib
    return lib


@contextlib.contextmanager
def knob(name, value):
    """Tests / diagnosis: run the block with one tuning knob of the library changed (mnerf_debug_set_knob)."""
    lib = load()
    old = C.c_int(0)
    check(lib.mnerf_debug_set_knob(name.encode(), int(value), C.byref(old)), "mnerf_debug_set_knob")
    try:
        yield
    finally:
        lib.mnerf_debug_set_knob(name.encode(), old.value, None)


def launch_plan(what, *args, n_plan=4):
    """Tests / diagnosis: the kernel instance the library would launch for a problem (mnerf_debug_launch_plan; include/mnerf.h lists
    the arguments and the values per dispatcher).  Needs no GPU.  -> tuple of ``n_plan`` ints."""
    lib = load()
    a = (C.c_int64 * len(args))(*[int(v) for v in args])
    plan = (C.c_int32 * n_plan)()
    check(lib.mnerf_debug_launch_plan(what.encode(), a, len(args), plan, n_plan), "mnerf_debug_launch_plan")
    return tuple(plan)


def check(rc, what):
    if rc != 0:
        msg = load().mnerf_last_error().decode(errors="replace")
        raise MnerfError(f"{what} failed (rc={rc}): {msg}")


# ----------------------------------------------------------------------- struct builders


def _fill(arr, values):
    flat = np.asarray(values, dtype=np.float32).reshape(-1)
    assert flat.size == len(arr), (flat.size, len(arr))
    for i, x in enumerate(flat):
        arr[i] = float(x)


def make_view(extr34, intr33, near, far):
    v = View()
    _fill(v.extr, extr34)
    _fill(v.intr, intr33)
    v.near_, v.far_ = float(near), float(far)
    return v


def make_rays(n_rays, n_samples, height, width, kinv, c2w, near, far, ray_begin=0, legacy=True,
              depth_inverse=False, ray_idx_ptr=None, strat_u_ptr=None, pose_table_ptr=None, rays_per_pose=0, tgt_hw=None):
    """``height`` / ``width``: the SOURCE views' size.  ``tgt_hw`` = (h, w): the pixel grid of the target the rays are cast through
    (``kinv``, ``ray_begin`` and a ``ray_idx`` list belong to it); None leaves the fields 0 = the views' size (include/mnerf.h:
    TARGET GRID).
    ``pose_table_ptr`` / ``rays_per_pose``: several target poses in one launch (include/mnerf.h: POSE TABLE; rows from
    ``pose_table_rows``); kinv / c2w / near / far are then ignored (pass those of any pose)."""
    r = Rays()
    if tgt_hw is not None:
        r.tgt_height, r.tgt_width = int(tgt_hw[0]), int(tgt_hw[1])
    r.pose_table = pose_table_ptr
    r.rays_per_pose = int(rays_per_pose) if pose_table_ptr else 0
    r.n_rays, r.n_samples, r.ray_begin = int(n_rays), int(n_samples), int(ray_begin)
    r.legacy_coord, r.depth_inverse = int(bool(legacy)), int(bool(depth_inverse))
    r.height, r.width = int(height), int(width)
    r.ray_idx = ray_idx_ptr
    r.strat_u = strat_u_ptr
    _fill(r.kinv, kinv)
    _fill(r.c2w, c2w)
    r.near_, r.far_ = float(near), float(far)
    return r


def pose_table_rows(poses):
    """[(kinv [3,3], c2w [3,4], near, far), ...] -> float32 [n, MNERF_POSE_FLOATS] rows of mnerf_rays.pose_table"""
    rows = np.zeros((len(poses), MNERF_POSE_FLOATS), np.float32)
    for i, (kinv, c2w, near, far) in enumerate(poses):
        rows[i, :9] = np.asarray(kinv, np.float32).reshape(-1)
        rows[i, 9:21] = np.asarray(c2w, np.float32).reshape(-1)
        rows[i, 21], rows[i, 22] = near, far
    return rows


@contextlib.contextmanager
def _on(device, stream=None):
    """Make ``device`` the current HIP device for the launch and yield the stream handle to launch on
    (``stream`` or that device's current torch stream)."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise MnerfError(f"the HIP kernels need CUDA tensors, got device {device} (there is no CPU fallback)")
    with torch.cuda.device(device):
        st = stream if stream is not None else torch.cuda.current_stream(device)
        yield C.c_void_p(st.cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_i32(t):
    """a device tensor of int32 for a parameter the header types as int32_t*"""
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_int32)) if t is not None else None


def _f32c(t, name):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise MnerfError(f"{name}: expected a contiguous float32 CUDA tensor, got {t.dtype} "
                         f"contig={t.is_contiguous()} device={t.device}")
    return t


def _current_device():
    import torch
    if not torch.cuda.is_available():
        raise MnerfError("the HIP kernels need a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------- op wrappers


def ray_samples(rays, view, device=None, stream=None):
    """a8-a10 (camera.py:255-286, 351-379) -> pts [R,S,3], ndc [R,S,3], depth [R,S]."""
    import torch
    lib = load()
    device = torch.device(device) if device is not None else _current_device()
    r, s = rays.n_rays, rays.n_samples
    pts = torch.empty(r, s, 3, device=device)
    ndc = torch.empty(r, s, 3, device=device)
    depth = torch.empty(r, s, device=device)
    with _on(device, stream) as st:
        check(lib.mnerf_ray_samples(C.byref(rays), C.byref(view), _ptr(pts), _ptr(ndc), _ptr(depth), st),
              "mnerf_ray_samples")
    return pts, ndc, depth


def composite(rgb_s, sigma, depth_s, ray_len=None, wo_render_interval=True, setbg_opaque=False, want_prob=False,
              stream=None):
    """K5 (nerf.py:101-124). rgb_s [R,S,3], sigma [R,S], depth_s [R,S] -> rgb [R,3], depth [R], opacity [R]
    (+ prob [R,S] with ``want_prob``)."""
    import torch
    lib = load()
    r, s = sigma.shape
    _f32c(rgb_s, "rgb_s"), _f32c(sigma, "sigma"), _f32c(depth_s, "depth_s")
    dev = sigma.device
    rgb = torch.empty(r, 3, device=dev)
    depth = torch.empty(r, device=dev)
    opacity = torch.empty(r, device=dev)
    prob = torch.empty(r, s, device=dev) if want_prob else None
    with _on(dev, stream) as st:
        check(lib.mnerf_composite(r, s, _ptr(rgb_s), _ptr(sigma), _ptr(depth_s), _ptr(ray_len),
                                  int(wo_render_interval), int(setbg_opaque), _ptr(rgb), _ptr(depth),
                                  _ptr(opacity), _ptr(prob), st), "mnerf_composite")
    if want_prob:
        return rgb, depth, opacity, prob
    return rgb, depth, opacity


def box_downsample(src, h, w, k, stream=None):
    """Box filter of a supersampled frame on the device (mnerf_box_downsample): src [k*h, k*w, C] or [k*h*k*w, C] fp32, C in
    {1, 3} (what ``render`` returns per batch element) -> [h, w, C].  Block sums in row-major order, times fp32(1 / k^2)."""
    import torch
    lib = load()
    _f32c(src, "src")
    h, w, k = int(h), int(w), int(k)
    c = int(src.shape[-1])
    if src.numel() != k * h * k * w * c:
        raise MnerfError(f"box_downsample: src {tuple(src.shape)} is not a [{k}*{h}, {k}*{w}, {c}] frame")
    dst = torch.empty(h, w, c, device=src.device)
    with _on(src.device, stream) as st:
        check(lib.mnerf_box_downsample(_ptr(src), h, w, c, k, _ptr(dst), st), "mnerf_box_downsample")
    return dst


def composite_backward(rgb_s, sigma, depth_s, g_rgb, g_depth=None, g_opacity=None, ray_len=None,
                       wo_render_interval=True, setbg_opaque=False, stream=None):
    """K5 backward: gradients of (rgb [R,3], depth [R], opacity [R]) -> (g_rgb_s [R,S,3], g_sigma [R,S])."""
    import torch
    lib = load()
    r, s = sigma.shape
    for t, n in ((rgb_s, "rgb_s"), (sigma, "sigma"), (depth_s, "depth_s"), (g_rgb, "g_rgb")):
        _f32c(t, n)
    g_rgb_s = torch.empty(r, s, 3, device=sigma.device)
    g_sigma = torch.empty(r, s, device=sigma.device)
    with _on(sigma.device, stream) as st:
        check(lib.mnerf_composite_backward(r, s, _ptr(rgb_s), _ptr(sigma), _ptr(depth_s), _ptr(ray_len),
                                           int(wo_render_interval), int(setbg_opaque), _ptr(g_rgb), _ptr(g_depth),
                                           _ptr(g_opacity), _ptr(g_rgb_s), _ptr(g_sigma), st), "mnerf_composite_backward")
    return g_rgb_s, g_sigma


def cost_volume_backward(scene, rays, cond_stride, g_cond, g_feats, stream=None):
    """K1+K2 backward: scatter-adds the gradient of the conditioning rows [n_rays*S, cond_stride] into ``g_feats``
    (list of 1 or 2 zero-initialised tensors shaped like the scene's feature maps)."""
    lib = load()
    _f32c(g_cond, "g_cond")
    for g in g_feats:
        _f32c(g, "g_feat")
    with _on(g_cond.device, stream) as st:
        check(lib.mnerf_cost_volume_backward(C.byref(scene), C.byref(rays), int(cond_stride), _ptr(g_cond),
                                             _ptr(g_feats[0]), _ptr(g_feats[1]) if len(g_feats) > 1 else None, st),
              "mnerf_cost_volume_backward")
    return g_feats


def decoder_backward(opt, params, n_views, x_ndc, dirs, cond, cond_stride, g_rgb_s, g_sigma, want_g_cond=True, raytrans_table=None,
                     grads=None, stream=None):
    """K3+K4 backward (cond_nerf.py:52-100 and ray_transformer.py:29-79 under autograd): ``params`` maps DEC_TRAIN_TENSORS names to
    fp32 CUDA tensors in torch's layouts; returns (g_cond [N, cond_stride] or None, {name: gradient}).  ``grads`` may hold
    tensors to accumulate into (missing names get fresh zero tensors; a name mapped to None is skipped)."""
    import torch
    lib = load()
    r, s = g_sigma.shape
    n = r * s
    dev = g_sigma.device
    for t, nm in ((x_ndc, "x_ndc"), (dirs, "dirs"), (cond, "cond"), (g_rgb_s, "g_rgb_s"), (g_sigma, "g_sigma")):
        _f32c(t, nm)
    d = DecoderTrain()
    dc = sum(opt.encoder.cos_n_group) + 4 * n_views
    skip = list(opt.decoder.skip)
    if len(skip) > 1:
        raise NotImplementedError("decoder_backward: one skip connection (opt.decoder.skip has %d)" % len(skip))
    d.n_views, d.cond_dim, d.n_trunk, d.net_width = n_views, dc, int(opt.decoder.net_depth), int(opt.decoder.net_width)
    d.skip_layer = int(skip[0]) if skip else -1
    d.L_3D = int(opt.decoder.posenc.L_3D) if opt.decoder.posenc else 0
    d.legacy_coord = int(bool(opt.nerf.legacy_coord))
    d.raytrans_elu = int(opt.decoder.raytrans_act == "ELU")
    d.raytrans_posenc = int(bool(opt.decoder.raytrans_posenc))
    d.density_maskfill = int(bool(opt.decoder.density_maskfill))
    keep = []
    if d.raytrans_posenc:
        tab = raytrans_table.to(dev).float().contiguous()
        keep.append(tab)
        d.raytrans_table = _ptr(tab)
    out = {}
    for k, name in enumerate(DEC_TRAIN_TENSORS):
        w = _f32c(params[name], name)
        keep.append(w)
        d.w[k] = _ptr(w)
        if grads is not None and name in grads:
            gk = grads[name]
        else:
            gk = torch.zeros_like(w)
        if gk is not None:
            _f32c(gk, "grad " + name)
            out[name] = gk
        d.g[k] = _ptr(gk)
    g_cond = torch.zeros(n, cond_stride, device=dev) if want_g_cond else None
    ws = _grow_only_workspace(dev, lib.mnerf_decoder_backward_workspace_bytes(r, s) // 4, stream)
    with _on(dev, stream) as st:
        check(lib.mnerf_decoder_backward(C.byref(d), r, s, _ptr(x_ndc), _ptr(dirs), _ptr(cond), int(cond_stride), _ptr(g_rgb_s),
                                         _ptr(g_sigma), _ptr(g_cond), _ptr(ws), st), "mnerf_decoder_backward")
    return g_cond, out


_BWD_WS = {}


def _grow_only_workspace(dev, n_floats, stream=None):
    """Scratch of the backward kernels, kept per (device, stream) and only ever grown: one allocation per process instead of one
    torch.empty per chunk and batch element.  SHARED by mnerf_decoder_backward (10.4 KB per sample: 0.7 GB for 1 024 rays x 64
    samples) and mnerf_encoder_layer_backward (about 0.5 GB at the DTU shape): the kernels of a call are enqueued on one stream
    in order and the next call's kernels follow them on that stream, so reuse needs no extra synchronisation.
    An explicit `stream` is not torch's current stream: the buffer is then allocated UNDER that stream and every use is recorded
    on it (Tensor.record_stream), so a buffer dropped when the scratch grows is not handed to another stream's allocation while
    kernels on `stream` still use it.  `release_workspaces()` frees the cache (it also goes with torch.cuda.empty_cache() once
    released); MNERF_BWD_WS_CAP_MB caps what is KEPT between calls (a larger request is served by a one-off buffer)."""
    import torch
    cur = torch.cuda.current_stream(dev)
    st = stream if stream is not None else cur
    key = (torch.device(dev), st.cuda_stream)
    buf = _BWD_WS.get(key)
    if buf is None or buf.numel() < n_floats:
        with torch.cuda.stream(st):
            buf = torch.empty(n_floats, device=dev)
        cap = float(os.environ.get("MNERF_BWD_WS_CAP_MB", "0") or 0)
        if cap <= 0 or n_floats * 4 <= cap * 2 ** 20:
            _BWD_WS[key] = buf
    if st.cuda_stream != cur.cuda_stream:
        buf.record_stream(st)
    return buf


def release_workspaces():
    """Drop the cached backward scratch buffers (they return to torch's caching allocator; torch.cuda.empty_cache() then
    gives the memory back to the driver)."""
    _BWD_WS.clear()


def cost_volume(scene, rays, cond_stride, out=None, device=None, stream=None):
    """K1+K2 (matchnerf.py:209-293) -> cond [n_rays*S, cond_stride].  The launch device is ``out``'s, else
    ``device``, else the current one (it must be where the scene's maps live)."""
    import torch
    lib = load()
    n = rays.n_rays * rays.n_samples
    if out is None:
        out = torch.empty(n, cond_stride, device=torch.device(device) if device is not None else _current_device())
    with _on(out.device, stream) as st:
        check(lib.mnerf_cost_volume(C.byref(scene), C.byref(rays), int(cond_stride), _ptr(out), st),
              "mnerf_cost_volume")
    return out


def cost_volume_operand_bytes(scene):
    """Bytes of the operand image of a scene's feature maps (mnerf_cost_volume_operands)."""
    n = int(load().mnerf_cost_volume_operand_bytes(C.byref(scene)))
    if n < 0:
        raise MnerfError("mnerf_cost_volume_operand_bytes: unsupported scene")
    return n


def cost_volume_operands(scene, out=None, device=None, stream=None):
    """The split-fp16 operand image of ``scene.feat`` for the matrix form of the cost volume (ABI v9): returns the uint8
    tensor that holds it and points ``scene.feat_op`` at it.  The caller keeps the tensor alive as long as the scene is used."""
    import torch
    lib = load()
    n = cost_volume_operand_bytes(scene)
    if out is None or out.numel() < n:
        out = torch.empty(n, dtype=torch.uint8, device=torch.device(device) if device is not None else _current_device())
    with _on(out.device, stream) as st:
        check(lib.mnerf_cost_volume_operands(C.byref(scene), _ptr(out), st), "mnerf_cost_volume_operands")
    scene.feat_op = out.data_ptr()
    return out


def decoder_chunk(dec, view0, rays, cond, want_samples=False, stream=None):
    """K3+K4+K5 (cond_nerf.py:52-100, ray_transformer.py, nerf.py:101-124)."""
    import torch
    lib = load()
    r, s = rays.n_rays, rays.n_samples
    dev = cond.device
    rgb = torch.empty(r, 3, device=dev)
    depth = torch.empty(r, device=dev)
    opacity = torch.empty(r, device=dev)
    rgb_s = torch.empty(r, s, 3, device=dev) if want_samples else None
    sigma = torch.empty(r, s, device=dev) if want_samples else None
    with _on(dev, stream) as st:
        check(lib.mnerf_decoder_chunk(C.byref(dec), C.byref(view0), C.byref(rays), _ptr(cond), _ptr(rgb),
                                      _ptr(depth), _ptr(opacity), _ptr(rgb_s), _ptr(sigma), st),
              "mnerf_decoder_chunk")
    if want_samples:
        return rgb, depth, opacity, rgb_s, sigma
    return rgb, depth, opacity


def decoder_samples(dec, x_ndc, dirs, cond, legacy_coord=True, stream=None):
    """K3+K4 with caller-supplied inputs (the literal CondNeRF.forward, cond_nerf.py:52-100):
    x_ndc [R,S,3], dirs [R,S,3], cond [R*S, cond_stride] -> rgb_s [R,S,3], sigma [R,S]."""
    import torch
    lib = load()
    _f32c(x_ndc, "x_ndc"), _f32c(dirs, "dirs"), _f32c(cond, "cond")
    r, s, _ = x_ndc.shape
    if tuple(dirs.shape) != (r, s, 3) or cond.numel() != r * s * dec.cond_stride:
        raise MnerfError(f"decoder_samples: x_ndc {tuple(x_ndc.shape)}, dirs {tuple(dirs.shape)}, cond "
                         f"{tuple(cond.shape)} (stride {dec.cond_stride}) do not agree")
    dev = x_ndc.device
    rgb_s = torch.empty(r, s, 3, device=dev)
    sigma = torch.empty(r, s, device=dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_decoder_samples(C.byref(dec), r, s, int(bool(legacy_coord)), _ptr(x_ndc), _ptr(dirs),
                                        _ptr(cond), _ptr(rgb_s), _ptr(sigma), st), "mnerf_decoder_samples")
    return rgb_s, sigma


class KernelTimer:
    """Per-kernel device timing with events recorded on the launch stream (bench.py roofline).
    ``spans[name]`` collects (start_event, end_event, n_rays) triples; ``summary`` syncs once."""

    def __init__(self):
        self.spans = {}

    def span(self, name, n_rays):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.spans.setdefault(name, []).append((e0, e1, n_rays))
        return e0, e1

    def reset(self):
        self.spans = {}

    def summary(self):
        out = {}
        for spans in self.spans.values():
            for _, end, _ in spans:
                end.synchronize()
        for name, spans in self.spans.items():
            ms = [a.elapsed_time(b) for a, b, _ in spans]
            out[name] = dict(launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / max(len(ms), 1),
                             rays=sum(n for _, _, n in spans))
        return out


def render_is_fused(scene, dec, rays):
    """True when the one-launch form of the ray chunk (mnerf_render_chunk_fused) exists for this configuration."""
    return bool(load().mnerf_render_chunk_is_fused(C.byref(scene), C.byref(dec), C.byref(rays)))


def render_takes_pose_table(scene, dec, n_samples, rays_per_pose):
    """True when a ray chunk of this scene / decoder may carry several target poses (``make_rays(pose_table_ptr=...)``)."""
    return bool(load().mnerf_render_takes_pose_table(C.byref(scene), C.byref(dec), int(n_samples), int(rays_per_pose)))


def render_chunk(scene, dec, rays, workspace, rgb, depth, opacity, stream=None, timer=None, fused=False):
    """a7 (matchnerf.py:88-143): writes rgb [R,3], depth [R], opacity [R] in place.
    ``fused=False`` (default, the faster form on MI355X): cost volume -> ``workspace`` -> decoder, two launches;
    with ``timer`` they go through their own entry points with spans "cost_volume" and "decoder".
    ``fused=True``: mnerf_render_chunk_fused, ONE launch, conditioning rows stay in LDS, ``workspace`` may be None
    (span "render_fused"); raises MnerfError where that form does not exist (``render_is_fused``)."""
    import torch
    lib = load()
    with _on(rgb.device, stream) as st:
        tst = stream if stream is not None else torch.cuda.current_stream(rgb.device)
        if fused:
            if timer is not None:
                e0, e1 = timer.span("render_fused", rays.n_rays)
                e0.record(tst)
            check(lib.mnerf_render_chunk_fused(C.byref(scene), C.byref(dec), C.byref(rays), _ptr(rgb), _ptr(depth),
                                               _ptr(opacity), st), "mnerf_render_chunk_fused")
            if timer is not None:
                e1.record(tst)
            return
        if timer is None:
            check(lib.mnerf_render_chunk(C.byref(scene), C.byref(dec), C.byref(rays), _ptr(workspace), _ptr(rgb),
                                         _ptr(depth), _ptr(opacity), st), "mnerf_render_chunk")
            return
        a0, a1 = timer.span("cost_volume", rays.n_rays)
        a0.record(tst)
        check(lib.mnerf_cost_volume(C.byref(scene), C.byref(rays), dec.cond_stride, _ptr(workspace), st),
              "mnerf_cost_volume")
        a1.record(tst)
        b0, b1 = timer.span("decoder", rays.n_rays)
        b0.record(tst)
        check(lib.mnerf_decoder_chunk(C.byref(dec), C.byref(scene.views[0]), C.byref(rays), _ptr(workspace),
                                      _ptr(rgb), _ptr(depth), _ptr(opacity), None, None, st), "mnerf_decoder_chunk")
        b1.record(tst)


def render_workspace_bytes(n_rays, n_samples, cond_stride):
    return int(load().mnerf_render_workspace_bytes(n_rays, n_samples, cond_stride))


# ----------------------------------------------------------------------- caller-supplied rays (include/mnerf.h)


def make_free_rays(n_rays, n_samples, height, width, near, far, legacy=True, depth_inverse=False, strat_u_ptr=None):
    """The mnerf_rays of a launch over a ray bundle: only the fields those entry points read (``height`` / ``width``: the SOURCE
    views' size; the sample parameters t come from near / far / n_samples as for pixel rays)."""
    return make_rays(n_rays, n_samples, height, width, np.zeros(9, np.float32), np.zeros(12, np.float32), near, far, legacy=legacy,
                     depth_inverse=depth_inverse, strat_u_ptr=strat_u_ptr)


def _bundle(ray_od, n_rays):
    _f32c(ray_od, "ray_od")
    if ray_od.numel() < n_rays * MNERF_RAY_FLOATS:
        raise MnerfError(f"ray_od {tuple(ray_od.shape)} holds fewer than {n_rays} rows of {MNERF_RAY_FLOATS} floats")
    return ray_od


def camera_rays(cam, pixel_begin=0, n_pixels=None, out=None, device=None, stream=None):
    """Rows of a ray bundle for pixels [pixel_begin, pixel_begin + n_pixels) of a camera model (``camera.camera_model``;
    mnerf_camera_rays) -> [n_pixels, 8] fp32 on the device: ox oy oz 0 | dx dy dz 0."""
    import torch
    lib = load()
    if n_pixels is None:
        n_pixels = cam.height * cam.width - int(pixel_begin)
    if out is None:
        out = torch.empty(int(n_pixels), MNERF_RAY_FLOATS, device=torch.device(device) if device is not None else _current_device())
    _bundle(out, int(n_pixels))
    with _on(out.device, stream) as st:
        check(lib.mnerf_camera_rays(C.byref(cam), int(pixel_begin), int(n_pixels), _ptr(out), st), "mnerf_camera_rays")
    return out


def cost_volume_rays(scene, rays, ray_od, cond_stride, out=None, stream=None):
    """K1+K2 over a ray bundle (mnerf_cost_volume_rays) -> cond [n_rays*S, cond_stride]: the rows of ``cost_volume``."""
    import torch
    lib = load()
    _bundle(ray_od, rays.n_rays)
    if out is None:
        out = torch.empty(rays.n_rays * rays.n_samples, cond_stride, device=ray_od.device)
    with _on(ray_od.device, stream) as st:
        check(lib.mnerf_cost_volume_rays(C.byref(scene), C.byref(rays), _ptr(ray_od), int(cond_stride), _ptr(out), st),
              "mnerf_cost_volume_rays")
    return out


def ray_samples_rays(rays, ray_od, view0, stream=None):
    """Per-sample geometry of a bundle (mnerf_ray_samples_rays) -> x_ndc [R,S,3], dir [R,S,3], depth_s [R,S], ray_len [R]."""
    import torch
    lib = load()
    _bundle(ray_od, rays.n_rays)
    r, s, dev = rays.n_rays, rays.n_samples, ray_od.device
    x_ndc, dirs = torch.empty(r, s, 3, device=dev), torch.empty(r, s, 3, device=dev)
    depth_s, ray_len = torch.empty(r, s, device=dev), torch.empty(r, device=dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_ray_samples_rays(C.byref(rays), _ptr(ray_od), C.byref(view0), _ptr(x_ndc), _ptr(dirs), _ptr(depth_s),
                                         _ptr(ray_len), st), "mnerf_ray_samples_rays")
    return x_ndc, dirs, depth_s, ray_len


def render_rays_workspace_bytes(n_rays, n_samples, cond_stride):
    return int(load().mnerf_render_rays_workspace_bytes(int(n_rays), int(n_samples), int(cond_stride)))


def render_rays_workspace_views(workspace, n_rays, n_samples, cond_stride):
    """The areas of a ``render_rays`` workspace (a float32 tensor) as views, in the layout include/mnerf.h documents:
    cond | x_ndc | dir | depth_s | rgb_s | sigma | ray_len, each area starting 16-byte aligned."""
    n = n_rays * n_samples
    out, at = {}, 0
    for name, count, shape in (("cond", n * cond_stride, (n, cond_stride)), ("x_ndc", n * 3, (n_rays, n_samples, 3)),
                               ("dir", n * 3, (n_rays, n_samples, 3)), ("depth_s", n, (n_rays, n_samples)),
                               ("rgb_s", n * 3, (n_rays, n_samples, 3)), ("sigma", n, (n_rays, n_samples)),
                               ("ray_len", n_rays, (n_rays,))):
        out[name] = workspace[at:at + count].view(shape)
        at += (count + 3) & ~3
    assert at * 4 == render_rays_workspace_bytes(n_rays, n_samples, cond_stride), (at, n_rays, n_samples, cond_stride)
    return out


def render_rays(scene, dec, rays, ray_od, workspace, rgb, depth, opacity, stream=None):
    """One render chunk over a ray bundle (mnerf_render_rays): writes rgb [R,3], depth [R], opacity [R] in place; the per-sample
    stages stay in ``workspace`` (``render_rays_workspace_views``)."""
    lib = load()
    _bundle(ray_od, rays.n_rays)
    with _on(rgb.device, stream) as st:
        check(lib.mnerf_render_rays(C.byref(scene), C.byref(dec), C.byref(rays), _ptr(ray_od), _ptr(workspace), _ptr(rgb),
                                    _ptr(depth), _ptr(opacity), st), "mnerf_render_rays")


def wa_math():
    """Matrix arithmetic of the window-attention kernel, MNERF_WA_MATH =
      'f16pre' (default)  split-fp16 products, K / V operand fragments + tile gains prepared once per call
      'f16x3'             the same arithmetic, every wave splits the K / V tiles itself (slower: 229 us per call)
      'bf16x6'            split-bf16, six products per MAC (204 us per call at 64x80 tokens)
      'f32'               exact-f32 MFMA"""
    m = os.environ.get("MNERF_WA_MATH", "f16pre")
    table = {"f16pre": WA_PRESPLIT_F16, "f16x3": WA_SPLIT_F16, "bf16x6": WA_SPLIT_BF16, "f32": WA_EXACT_F32}
    if m not in table:
        raise ValueError(f"MNERF_WA_MATH={m!r}: expected one of {sorted(table)}")
    return table[m]


def _wa_check_row_stats(what, row_stats, n_tokens):
    import torch
    if tuple(row_stats.shape) != (2, n_tokens) or row_stats.dtype != torch.float32 or not row_stats.is_contiguous():
        raise MnerfError(f"{what}: row_stats must be a contiguous float32 [2, {n_tokens}] tensor")


def _wa_workspace(nbytes, device, stream):
    """scratch of one attention call, at least 16 bytes, in use on ``stream`` (the caching allocator's: no hipMalloc)"""
    import torch
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    if stream is not None:
        ws.record_stream(stream)
    return ws


def window_attention(q, k, v, h, w, num_splits, shifted, out=None, math=None, stream=None, row_stats=None):
    """K6 (gmflow/transformer.py:8-105). q,k,v [B,h*w,128] -> [B,h*w,128].  ``row_stats`` (training forward, default arithmetic
    only): a float32 [2, B*h*w] tensor that receives the softmax's row statistics for ``window_attention_backward``."""
    import torch
    lib = load()
    _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
    b, n, c = q.shape
    if c != 128 or n != h * w:
        raise MnerfError(f"window_attention: expected [B,{h * w},128], got {tuple(q.shape)}")
    if out is None:
        out = torch.empty_like(q)
    math = wa_math() if math is None else int(math)
    with _on(q.device, stream) as st:
        if math == WA_PRESPLIT_F16:
            nbytes = int(lib.mnerf_window_attention_workspace_bytes(b, h, w, int(num_splits)))
            ws = _wa_workspace(nbytes, q.device, stream)
            if row_stats is not None:
                _wa_check_row_stats("window_attention", row_stats, b * n)
                check(lib.mnerf_window_attention_presplit_stats(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(row_stats), b, h, w,
                                                                int(num_splits), int(bool(shifted)), _ptr(ws), nbytes, st),
                      "mnerf_window_attention_presplit_stats")
                return out
            check(lib.mnerf_window_attention_presplit(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, h, w, int(num_splits),
                                                      int(bool(shifted)), _ptr(ws), nbytes, st),
                  "mnerf_window_attention_presplit")
        elif row_stats is not None:
            raise MnerfError("window_attention: row_stats needs the default arithmetic (MNERF_WA_MATH=f16pre)")
        else:
            check(lib.mnerf_window_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, h, w, int(num_splits),
                                             int(bool(shifted)), math, st), "mnerf_window_attention")
    return out


def window_attention_backward(q, k, v, out, g_out, h, w, num_splits, shifted, stream=None, row_stats=None):
    """K6 backward (mnerf_window_attention_backward): gradients of q, k, v [B,h*w,128] given the forward's ``out`` and its
    gradient ``g_out``; flash style (no score tensor), fp32-grade, deterministic.  ``row_stats``: what ``window_attention``
    filled in the forward (the statistics pass is skipped)."""
    import torch
    lib = load()
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (g_out, "g_out")):
        _f32c(t, name)
    b, n, c = q.shape
    if c != 128 or n != h * w or any(tuple(t.shape) != (b, n, c) for t in (k, v, out, g_out)):
        raise MnerfError(f"window_attention_backward: expected five [B,{h * w},128] tensors, got {tuple(q.shape)} ...")
    g_q, g_k, g_v = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    ws = _wa_workspace(lib.mnerf_window_attention_backward_workspace_bytes(b, h, w), q.device, stream)
    with _on(q.device, stream) as st:
        if row_stats is not None:
            _wa_check_row_stats("window_attention_backward", row_stats, b * n)
            check(lib.mnerf_window_attention_backward_stats(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(g_out), _ptr(row_stats), _ptr(g_q),
                                                            _ptr(g_k), _ptr(g_v), b, h, w, int(num_splits), int(bool(shifted)),
                                                            _ptr(ws), ws.numel(), st), "mnerf_window_attention_backward_stats")
            return g_q, g_k, g_v
        check(lib.mnerf_window_attention_backward(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(g_out), _ptr(g_q), _ptr(g_k), _ptr(g_v),
                                                  b, h, w, int(num_splits), int(bool(shifted)), _ptr(ws),
                                                  ws.numel(), st), "mnerf_window_attention_backward")
    return g_q, g_k, g_v


def qkv_projection(wstream, ews, x_q, x_kv=None, kv_swap=False, stream=None):
    """q, k, v = Wq x_q, Wk x_kv', Wv x_kv' of a GMFlow transformer layer in one launch (transformer.py:147-151);
    x_* [n_seq, seq_len, 128]; ``kv_swap``: x_kv' = x_kv with its batch halves exchanged.  wstream / ews from
    gmflow.pack_qkv."""
    import torch
    lib = load()
    x_kv = x_q if x_kv is None else x_kv
    _f32c(x_q, "x_q"), _f32c(x_kv, "x_kv"), _f32c(wstream, "wstream")
    if x_q.dim() != 3 or x_q.shape[2] != 128 or x_kv.shape != x_q.shape:
        raise MnerfError(f"qkv_projection: expected two [n_seq, seq_len, 128] tensors, got {tuple(x_q.shape)}, {tuple(x_kv.shape)}")
    if wstream.numel() != lib.mnerf_qkv_wstream_floats():
        raise MnerfError(f"qkv_projection: wstream has {wstream.numel()} floats, expected {lib.mnerf_qkv_wstream_floats()}")
    q, k, v = (torch.empty_like(x_q) for _ in range(3))
    ew = (C.c_int32 * 3)(*[int(e) for e in ews])
    with _on(x_q.device, stream) as st:
        check(lib.mnerf_qkv_projection(_ptr(wstream), ew, _ptr(x_q), _ptr(x_kv), int(bool(kv_swap)), _ptr(q), _ptr(k),
                                       _ptr(v), x_q.shape[0], x_q.shape[1], st), "mnerf_qkv_projection")
    return q, k, v


def qkv_window_images(wstream, ews, x_q, x_kv, kv_swap, h, w, num_splits, shifted, stream=None):
    """q|k|v projections with K and V written as the window attention's operand images (csrc/qkv.hip).
    -> (q [B,h*w,128], workspace) for ``window_attention_images`` with the same geometry."""
    import torch
    lib = load()
    x_kv = x_q if x_kv is None else x_kv
    _f32c(x_q, "x_q"), _f32c(x_kv, "x_kv"), _f32c(wstream, "wstream")
    b, n, c = x_q.shape
    if c != 128 or n != h * w or x_kv.shape != x_q.shape:
        raise MnerfError(f"qkv_window_images: expected two [B,{h * w},128] tensors, got {tuple(x_q.shape)}, {tuple(x_kv.shape)}")
    if wstream.numel() != lib.mnerf_qkv_wstream_floats():
        raise MnerfError(f"qkv_window_images: wstream has {wstream.numel()} floats, expected {lib.mnerf_qkv_wstream_floats()}")
    q = torch.empty_like(x_q)
    nbytes = int(lib.mnerf_window_attention_workspace_bytes(b, h, w, int(num_splits)))
    ws = _wa_workspace(nbytes, x_q.device, stream)
    ew = (C.c_int32 * 3)(*[int(e) for e in ews])
    with _on(x_q.device, stream) as st:
        check(lib.mnerf_qkv_window_images(_ptr(wstream), ew, _ptr(x_q), _ptr(x_kv), int(bool(kv_swap)), _ptr(q),
                                          _ptr(ws), nbytes, b, h, w, int(num_splits), int(bool(shifted)), st),
              "mnerf_qkv_window_images")
    return q, ws


def window_attention_images(q, workspace, h, w, num_splits, shifted, out=None, stream=None):
    """K6 on K / V operand images prepared by ``qkv_window_images`` (same geometry arguments)."""
    import torch
    lib = load()
    _f32c(q, "q")
    b, n, c = q.shape
    if c != 128 or n != h * w:
        raise MnerfError(f"window_attention_images: expected [B,{h * w},128], got {tuple(q.shape)}")
    if out is None:
        out = torch.empty_like(q)
    with _on(q.device, stream) as st:
        check(lib.mnerf_window_attention_images(_ptr(q), _ptr(out), b, h, w, int(num_splits), int(bool(shifted)),
                                                _ptr(workspace), workspace.numel(), st),
              "mnerf_window_attention_images")
    return out


def encoder_layer_backward(layer, attn, source, g_out, grads, stream=None, saved=None):
    """Backward of everything after the attention in a transformer layer (mnerf_encoder_layer_backward).  ``layer``: the
    TransformerLayer module (merge / norm1 / mlp / norm2 parameters are read in torch's layouts); attn, source, g_out [N,128];
    ``grads``: dict parameter tensor -> gradient tensor to ACCUMULATE into (a missing entry skips that parameter).
    ``saved``: (m1 [N,128], z1 [N,1024], m2 [N,128]) as ``encoder_block(..., save=True)`` returned them (z1, m2 None without an FFN;
    mnerf_encoder_layer_backward_saved: the GEMMs that would re-evaluate them are skipped).  -> (g_attn, g_source) [N,128]."""
    import torch
    lib = load()
    for t, name in ((attn, "attn"), (source, "source"), (g_out, "g_out")):
        _f32c(t, name)
    n, c = source.shape
    if c != 128 or tuple(attn.shape) != (n, c) or tuple(g_out.shape) != (n, c):
        raise MnerfError(f"encoder_layer_backward: attn {tuple(attn.shape)}, source {tuple(source.shape)}, g_out {tuple(g_out.shape)}")
    L = EncoderLayerTrain()
    L.ffn = int(not layer.no_ffn)
    keep = []

    def put(field, p):
        w = p.detach()
        _f32c(w, field)
        keep.append(w)
        setattr(L, field, w.data_ptr())
        g = grads.get(p)
        if g is not None:
            _f32c(g, "grad " + field)
            if tuple(g.shape) != tuple(p.shape):
                raise MnerfError(f"encoder_layer_backward: gradient of {field} has shape {tuple(g.shape)}")
            setattr(L, "g_" + field, g.data_ptr())

    put("w_merge", layer.merge.weight), put("ln1_w", layer.norm1.weight), put("ln1_b", layer.norm1.bias)
    if not layer.no_ffn:
        put("w_mlp0", layer.mlp[0].weight), put("w_mlp2", layer.mlp[2].weight)
        put("ln2_w", layer.norm2.weight), put("ln2_b", layer.norm2.bias)
    g_attn, g_source = torch.empty_like(source), torch.empty_like(source)
    ws = _grow_only_workspace(source.device, int(lib.mnerf_encoder_layer_backward_workspace_bytes(n)) // 4, stream)
    with _on(source.device, stream) as st:
        if saved is not None:
            m1, z1, m2 = saved
            _f32c(m1, "m1")
            if tuple(m1.shape) != (n, 128):
                raise MnerfError(f"encoder_layer_backward: saved m1 {tuple(m1.shape)}")
            if layer.no_ffn:
                z1 = m2 = None
            else:
                _f32c(z1, "z1"), _f32c(m2, "m2")
                if tuple(z1.shape) != (n, 1024) or tuple(m2.shape) != (n, 128):
                    raise MnerfError(f"encoder_layer_backward: saved z1 {tuple(z1.shape)}, m2 {tuple(m2.shape)}")
            check(lib.mnerf_encoder_layer_backward_saved(C.byref(L), _ptr(attn), _ptr(source), _ptr(g_out), _ptr(m1), _ptr(z1), _ptr(m2),
                                                         _ptr(g_attn), _ptr(g_source), n, _ptr(ws), st),
                  "mnerf_encoder_layer_backward_saved")
            return g_attn, g_source
        check(lib.mnerf_encoder_layer_backward(C.byref(L), _ptr(attn), _ptr(source), _ptr(g_out), _ptr(g_attn), _ptr(g_source), n,
                                               _ptr(ws), st), "mnerf_encoder_layer_backward")
    return g_attn, g_source


def qkv_backward(w_q, w_k, w_v, x_q, x_kv, g_q, g_k, g_v, gw_q=None, gw_k=None, gw_v=None, stream=None):
    """Backward of the three bias-free projections (mnerf_qkv_backward): x_* and g_* [N,128], w_* [128,128];
    gw_* (optional) are ACCUMULATED into.  -> (g_xq, g_xkv) [N,128]."""
    import torch
    lib = load()
    ts = [w_q.detach(), w_k.detach(), w_v.detach(), x_q, x_kv, g_q, g_k, g_v]
    for t in ts:
        _f32c(t, "qkv_backward operand")
    n = x_q.shape[0]
    if any(tuple(t.shape) != (n, 128) for t in ts[3:]) or any(tuple(t.shape) != (128, 128) for t in ts[:3]):
        raise MnerfError("qkv_backward: expected [N,128] activations / gradients and [128,128] weights")
    g_xq, g_xkv = torch.empty_like(x_q), torch.empty_like(x_q)
    with _on(x_q.device, stream) as st:
        check(lib.mnerf_qkv_backward(*[_ptr(t) for t in ts], _ptr(g_xq), _ptr(g_xkv), _ptr(gw_q), _ptr(gw_k), _ptr(gw_v), n, st),
              "mnerf_qkv_backward")
    return g_xq, g_xkv


def debug_gemm(a, b, bias=None, out=None, mode=0, math="bf16x6", stream=None):
    """Test hook (mnerf_debug_gemm): C (mode 0: =, 1: +=, 2: atomic +=) a @ b (+ bias) for 2-D fp32 tensors of ANY strides (views and
    transposes go through as they are); ``math``: "bf16x6" (the library's default for products with I, J >= 128), "f16x3" (split-fp16 with row gains, round 6: selectable with MNERF_GEMM_MATH) or "f32"."""
    import torch
    lib = load()
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0] or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise MnerfError(f"debug_gemm: {tuple(a.shape)} @ {tuple(b.shape)}")
    I, K = a.shape
    J = b.shape[1]
    if out is None:
        out = torch.zeros(I, J, device=a.device)
    if out.stride(1) != 1:
        raise MnerfError("debug_gemm: out must have unit column stride")
    with _on(a.device, stream) as st:
        check(lib.mnerf_debug_gemm(_ptr(a), a.stride(0), a.stride(1), _ptr(b), b.stride(0), b.stride(1), _ptr(out), out.stride(0),
                                   _ptr(bias), I, J, K, int(mode), {"f32": 0, "bf16x6": 1, "f16x3": 2}[math], st), "mnerf_debug_gemm")
    return out


def instance_norm(x, residual=None, relu_inner=False, relu_outer=False, eps=1e-5, out=None, out_absmax=None, stream=None):
    """F.instance_norm(x) of an NCHW tensor fused with the ReLU / residual add / ReLU that follow it in the GMFlow
    backbone (backbone.py:27-35): out = [relu](residual + [relu](IN(x))).  ``out_absmax``: absmax region that max|out|
    is merged into (the operand scale of the convolution that reads ``out``)."""
    import torch
    lib = load()
    _f32c(x, "x")
    if x.dim() != 4:
        raise MnerfError(f"instance_norm: expected [N,C,H,W], got {tuple(x.shape)}")
    if residual is not None:
        _f32c(residual, "residual")
        if residual.shape != x.shape:
            raise MnerfError(f"instance_norm: residual {tuple(residual.shape)} vs x {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    n, c, h, w = x.shape
    with _on(x.device, stream) as st:
        check(lib.mnerf_instance_norm(_ptr(x), _ptr(residual), _ptr(out), n * c, h * w, float(eps), int(bool(relu_inner)),
                                      int(bool(relu_outer)), _ptr(out_absmax), st), "mnerf_instance_norm")
    return out


def absmax_regions(n, device):
    """n zeroed absmax regions [n, ABSMAX_FLOATS] (include/mnerf.h): the hand-over of a tensor's largest magnitude from
    the kernel that writes it to the split-fp16 convolution that reads it."""
    import torch
    return torch.zeros(n, ABSMAX_FLOATS, device=device, dtype=torch.float32)


def absmax_value(region):
    """the maximum an absmax region holds (device tensor, no sync)"""
    return region.max()


def absmax(x, out, stream=None):
    """max|x| merged into the absmax region ``out`` (atomic maxima: zero it first)."""
    lib = load()
    _f32c(x, "x")
    with _on(x.device, stream) as st:
        check(lib.mnerf_absmax(_ptr(x), x.numel(), _ptr(out), st), "mnerf_absmax")
    return out


def upsample_bilinear2x(x, add=None, stream=None):
    """F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) (+ add): [N,C,H,W] -> [N,C,2H,2W]."""
    import torch
    lib = load()
    _f32c(x, "x")
    n, c, h, w = x.shape
    out = torch.empty(n, c, 2 * h, 2 * w, device=x.device, dtype=torch.float32)
    if add is not None:
        _f32c(add, "add")
    with _on(x.device, stream) as st:
        check(lib.mnerf_upsample_bilinear2x(_ptr(x), _ptr(add), _ptr(out), n * c, h, w, st), "mnerf_upsample_bilinear2x")
    return out


def upsample_bilinear2x_backward(dout, stream=None):
    """the adjoint: [N,C,2H,2W] -> [N,C,H,W]"""
    import torch
    lib = load()
    _f32c(dout, "dout")
    n, c, h2, w2 = dout.shape
    din = torch.empty(n, c, h2 // 2, w2 // 2, device=dout.device, dtype=torch.float32)
    with _on(dout.device, stream) as st:
        check(lib.mnerf_upsample_bilinear2x_backward(_ptr(dout), _ptr(din), n * c, h2 // 2, w2 // 2, st), "mnerf_upsample_bilinear2x_backward")
    return din


def instance_norm_backward(x, dy, relu, eps=1e-5, stream=None):
    """dx of out = [relu](InstanceNorm2d(x)) (no affine): x, dy [N,C,H,W] -> [N,C,H,W] (csrc/instance_norm.hip)."""
    import torch
    lib = load()
    _f32c(x, "x"), _f32c(dy, "dy")
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    with _on(x.device, stream) as st:
        check(lib.mnerf_instance_norm_backward(_ptr(x), _ptr(dy), _ptr(dx), n * c, h * w, float(eps), int(bool(relu)), st),
              "mnerf_instance_norm_backward")
    return dx


def conv2d_backward_data(dy, weight, h_in, w_in, stride, stream=None):
    """dX of Conv2d(c_in, c_out, k, stride, padding=k//2) (csrc/conv_backward.hip).  dy [N,c_out,Ho,Wo], weight [c_out,c_in,k,k]
    -> [N,c_in,h_in,w_in]."""
    import torch
    lib = load()
    _f32c(dy, "dy")
    c_out, c_in, k, _ = weight.shape
    n = dy.shape[0]
    wt = weight.detach().permute(2, 3, 0, 1).contiguous()
    dx = torch.empty(n, c_in, h_in, w_in, device=dy.device, dtype=torch.float32)
    with _on(dy.device, stream) as st:
        check(lib.mnerf_conv2d_backward_data(_ptr(dy), _ptr(wt), _ptr(dx), n, c_in, c_out, int(h_in), int(w_in), int(k), int(stride), st),
              "mnerf_conv2d_backward_data")
    return dx


def conv2d_forward_f32(x, weight, bias, stride, stream=None):
    """Conv2d(c_in, c_out, k, stride, padding=k//2) in exact fp32 (the training forward; csrc/conv_backward.hip).
    x [N,c_in,H,W], weight [c_out,c_in,k,k] -> [N,c_out,Ho,Wo]."""
    import torch
    lib = load()
    _f32c(x, "x")
    c_out, c_in, k, _ = weight.shape
    n, _, h, w = x.shape
    wt = weight.detach().permute(2, 3, 1, 0).contiguous()
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    y = torch.empty(n, c_out, ho, wo, device=x.device, dtype=torch.float32)
    b = bias.detach().contiguous() if bias is not None else None
    with _on(x.device, stream) as st:
        check(lib.mnerf_conv2d_forward_f32(_ptr(x), _ptr(wt), _ptr(b), _ptr(y), n, c_in, c_out, h, w, int(k), int(stride), st),
              "mnerf_conv2d_forward_f32")
    return y


def conv_stem_backward_weight(x, dy, stream=None):
    """dW [64,3,7,7] of the stem Conv2d(3, 64, 7, 2, 3): x [N,3,H,W], dy [N,64,(H-1)//2+1,(W-1)//2+1]."""
    import torch
    lib = load()
    _f32c(x, "x"), _f32c(dy, "dy")
    n, _, h, w = x.shape
    nbytes = int(lib.mnerf_conv_stem_backward_weight_workspace_bytes(n, h, w))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    if stream is not None:
        ws.record_stream(stream)
    dw = torch.empty(64, 3, 7, 7, device=x.device, dtype=torch.float32)
    with _on(x.device, stream) as st:
        check(lib.mnerf_conv_stem_backward_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, n, h, w, st),
              "mnerf_conv_stem_backward_weight")
    return dw


def conv2d_backward_weight(x, dy, ksize, stride, x_absmax=None, dy_absmax=None, stream=None):
    """dW of the same convolution: x [N,c_in,H,W], dy [N,c_out,Ho,Wo] -> [c_out,c_in,k,k].  With the two absmax regions (max|x|,
    max|dy|): three split-fp16 products per MAC on the 16-bit matrix pipe; without: exact-f32 matrix products."""
    import torch
    lib = load()
    _f32c(x, "x"), _f32c(dy, "dy")
    n, c_in, h, w = x.shape
    c_out = dy.shape[1]
    nbytes = int(lib.mnerf_conv2d_backward_weight_workspace_bytes(n, c_in, c_out, h, w, int(ksize), int(stride)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    if stream is not None:
        ws.record_stream(stream)
    dw = torch.empty(c_out, c_in, ksize, ksize, device=x.device, dtype=torch.float32)
    with _on(x.device, stream) as st:
        if x_absmax is not None and dy_absmax is not None:
            check(lib.mnerf_conv2d_backward_weight_f16x3(_ptr(x), _ptr(dy), _ptr(x_absmax), _ptr(dy_absmax), _ptr(dw), _ptr(ws), nbytes, n,
                                                         c_in, c_out, h, w, int(ksize), int(stride), st), "mnerf_conv2d_backward_weight_f16x3")
        else:
            check(lib.mnerf_conv2d_backward_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), nbytes, n, c_in, c_out, h, w, int(ksize),
                                                   int(stride), st), "mnerf_conv2d_backward_weight")
    return dw


def conv_stem(x, wstream, ew, in_absmax, out=None, stream=None):
    """The backbone's 7x7 stride-2 stem (3 -> 64 channels, backbone.py:45) on the split-fp16 matrix path.
    x [N,3,H,W] -> [N,64,(H-1)//2+1,(W-1)//2+1]; wstream / ew from gmflow.pack_conv_stem."""
    import torch
    lib = load()
    _f32c(x, "x"), _f32c(wstream, "wstream")
    if x.dim() != 4 or x.shape[1] != 3:
        raise MnerfError(f"conv_stem: expected [N,3,H,W], got {tuple(x.shape)}")
    if wstream.numel() != lib.mnerf_conv_stem_wstream_floats():
        raise MnerfError(f"conv_stem: wstream has {wstream.numel()} floats, expected {lib.mnerf_conv_stem_wstream_floats()}")
    n, _, h, w = x.shape
    if out is None:
        out = torch.empty(n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1, device=x.device, dtype=torch.float32)
    with _on(x.device, stream) as st:
        check(lib.mnerf_conv_stem(_ptr(wstream), int(ew), _ptr(x), _ptr(in_absmax), _ptr(out), n, h, w, st), "mnerf_conv_stem")
    return out


def conv2d(x, wstream, bias, c_in, c_out, ksize, stride, ew, in_absmax, leaky=1.0, channels_last=False, upsample2x=False,
           add_bilinear2x=None, out_layout=CONV_OUT_NCHW, add_channel_last=None, out_absmax=None, out=None, stream=None):
    """Split-fp16 implicit-GEMM convolution (csrc/conv.hip; gmflow/backbone.py, superres.py).  x [N,c_in,H,W], or
    [N,H,W,c_in] with ``channels_last``; ``wstream`` from gmflow.pack_conv; ``in_absmax``: absmax region filled by the
    producer of x; ``add_bilinear2x`` [N,c_out,H_out/2,W_out/2]: its bilinear 2x up-sampling is added to the result.
    ``out_layout``: CONV_OUT_NCHW -> [N,c_out,H_out,W_out]; CONV_OUT_CHANNEL_LAST -> tokens [N,H_out,W_out,c_out]
    (+ ``add_channel_last`` [H_out*W_out, c_out] added to every image); CONV_OUT_PAIR_MAJOR -> the cost volume's layout
    [N/2,2,H_out,W_out,c_out]."""
    import torch
    lib = load()
    _f32c(x, "x"), _f32c(wstream, "wstream")
    if x.dim() != 4:
        raise MnerfError(f"conv2d: expected a 4-D tensor, got {tuple(x.shape)}")
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if channels_last else (x.shape[0], x.shape[2], x.shape[3])
    if (x.shape[3] if channels_last else x.shape[1]) != c_in:
        raise MnerfError(f"conv2d: input {tuple(x.shape)} does not have {c_in} channels")
    up = 1 if upsample2x else 0
    pad = ksize // 2
    h_out = ((h << up) + 2 * pad - ksize) // stride + 1
    w_out = ((w << up) + 2 * pad - ksize) // stride + 1
    if add_bilinear2x is not None:
        _f32c(add_bilinear2x, "add_bilinear2x")
        if tuple(add_bilinear2x.shape) != (n, c_out, h_out // 2, w_out // 2):
            raise MnerfError(f"conv2d: add_bilinear2x {tuple(add_bilinear2x.shape)} vs output {(n, c_out, h_out, w_out)}")
    if out is None:
        shape = {CONV_OUT_NCHW: (n, c_out, h_out, w_out), CONV_OUT_CHANNEL_LAST: (n, h_out, w_out, c_out),
                 CONV_OUT_PAIR_MAJOR: (n // 2, 2, h_out, w_out, c_out)}[out_layout]
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    if add_channel_last is not None:
        _f32c(add_channel_last, "add_channel_last")
        if add_channel_last.numel() != h_out * w_out * c_out:
            raise MnerfError(f"conv2d: add_channel_last {tuple(add_channel_last.shape)} vs {(h_out * w_out, c_out)}")
    cv = ConvLayer()
    cv.wstream, cv.wstream_floats = wstream.data_ptr(), wstream.numel()
    cv.bias = bias.data_ptr() if bias is not None else None
    cv.c_in, cv.c_out, cv.ksize, cv.stride, cv.ew, cv.leaky_slope = c_in, c_out, ksize, stride, int(ew), float(leaky)
    with _on(x.device, stream) as st:
        check(lib.mnerf_conv2d(C.byref(cv), _ptr(x), int(bool(channels_last)), up, _ptr(in_absmax), _ptr(add_bilinear2x),
                               _ptr(add_channel_last), _ptr(out), int(out_layout), _ptr(out_absmax), n, h, w, st),
              "mnerf_conv2d")
    return out


def encoder_block(attn, source, wstream, ln, ffn, ews, out=None, stream=None, save=False):
    """K7 (gmflow/transformer.py:176-185): out = source + norm2(mlp(cat[source, norm1(merge(attn))])) (or without the
    FFN).  attn, source [N,128]; wstream / ews from gmflow.pack_encoder_block; ln [4,128].  ``save`` (training): -> (out, m1 [N,128], z1 [N,1024],
    m2 [N,128]) - merge's output before norm1 and, with an FFN (None otherwise), mlp.0's output before the GELU and mlp.2's output
    before norm2 - for ``encoder_layer_backward(..., saved=(m1, z1, m2))`` (mnerf_encoder_block_save)."""
    import torch
    lib = load()
    _f32c(attn, "attn"), _f32c(source, "source"), _f32c(wstream, "wstream"), _f32c(ln, "ln")
    n, c = source.shape
    if c != 128 or tuple(attn.shape) != (n, c) or tuple(ln.shape) != (4, 128):
        raise MnerfError(f"encoder_block: attn {tuple(attn.shape)}, source {tuple(source.shape)}, ln {tuple(ln.shape)}")
    if out is None:
        out = torch.empty_like(source)
    blk = EncoderLayer()
    blk.wstream, blk.wstream_floats, blk.ln = wstream.data_ptr(), wstream.numel(), ln.data_ptr()
    blk.ffn, blk.ew_merge, blk.ew_w1, blk.ew_w2 = int(bool(ffn)), int(ews[0]), int(ews[1]), int(ews[2])
    with _on(source.device, stream) as st:
        if save:
            m1 = torch.empty(n, 128, device=source.device)
            z1 = torch.empty(n, 1024, device=source.device) if ffn else None
            m2 = torch.empty(n, 128, device=source.device) if ffn else None
            check(lib.mnerf_encoder_block_save(C.byref(blk), _ptr(attn), _ptr(source), _ptr(out), _ptr(m1), _ptr(z1), _ptr(m2), n, st),
                  "mnerf_encoder_block_save")
            return out, m1, z1, m2
        check(lib.mnerf_encoder_block(C.byref(blk), _ptr(attn), _ptr(source), _ptr(out), n, st), "mnerf_encoder_block")
    return out


# ----------------------------------------------------------------------- the tail of a training iteration (csrc/optim.hip)


def optim_groups(groups):
    """[(lr, beta1, beta2, eps, weight_decay, max_norm, n_blocks), ...] -> the by-value array of mnerf_optim_group"""
    if not 1 <= len(groups) <= OPTIM_MAX_GROUPS:
        raise MnerfError(f"optim_groups: {len(groups)} parameter groups, the kernels take 1..{OPTIM_MAX_GROUPS}")
    arr = (OptimGroup * len(groups))()
    for a, (lr, b1, b2, eps, wd, max_norm, n_blocks) in zip(arr, groups):
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(lr), float(b1), float(b2), float(eps), float(wd)
        a.max_norm, a.n_blocks = float(max_norm or 0.0), int(n_blocks)
    return arr


def grad_sumsq(rows, n_rows, n_blocks, groups, workspace, sumsq, stream=None):
    """Sum of squared gradients per parameter group, deterministic (mnerf_grad_sumsq).  ``rows``: uint8 CUDA tensor holding n_rows
    OptimRow records; ``groups``: from ``optim_groups``; ``workspace`` >= n_blocks floats; ``sumsq`` >= len(groups) floats."""
    lib = load()
    _f32c(workspace, "workspace"), _f32c(sumsq, "sumsq")
    if rows.numel() < n_rows * C.sizeof(OptimRow) or workspace.numel() < n_blocks or sumsq.numel() < len(groups):
        raise MnerfError("grad_sumsq: rows / workspace / sumsq too small for the table")
    with _on(rows.device, stream) as st:
        check(lib.mnerf_grad_sumsq(_ptr(rows), int(n_rows), int(n_blocks), groups, len(groups), _ptr(workspace), _ptr(sumsq), st),
              "mnerf_grad_sumsq")
    return sumsq


def adamw_step(rows, n_rows, n_blocks, groups, sumsq=None, stream=None):
    """Clip + AdamW over every row of the table in one launch (mnerf_adamw_step); ``sumsq`` from ``grad_sumsq`` when a group clips."""
    lib = load()
    if rows.numel() < n_rows * C.sizeof(OptimRow) or (sumsq is not None and sumsq.numel() < len(groups)):
        raise MnerfError("adamw_step: rows / sumsq too small for the table")
    with _on(rows.device, stream) as st:
        check(lib.mnerf_adamw_step(_ptr(rows), int(n_rows), int(n_blocks), groups, len(groups), _ptr(sumsq), st),
              "mnerf_adamw_step")


def l2_loss(pred, target, weight=1.0, want_grad=True, stream=None):
    """weight * mean((pred - target)^2) as a 0-d tensor and its gradient with respect to ``pred`` (or None), one launch, deterministic."""
    import torch
    lib = load()
    if not pred.is_cuda:
        raise MnerfError(f"l2_loss: the HIP kernels need CUDA tensors, got device {pred.device} (there is no CPU fallback)")
    _f32c(pred, "pred"), _f32c(target, "target")
    if pred.shape != target.shape or pred.numel() == 0 or pred.device != target.device:
        raise MnerfError(f"l2_loss: pred {tuple(pred.shape)} on {pred.device} vs target {tuple(target.shape)} on {target.device}")
    loss = torch.empty((), device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    with _on(pred.device, stream) as st:
        check(lib.mnerf_l2_loss(_ptr(pred), _ptr(target), pred.numel(), float(weight), _ptr(loss), _ptr(grad), st), "mnerf_l2_loss")
    return loss, grad


# ----------------------------------------------------------------------- the gradient exchange of data-parallel training


def grad_bucket_floats(n_blocks):
    """floats of the bucket of a row table of ``n_blocks`` chunks: the chunks plus one chunk of side slots (host only)"""
    return (int(n_blocks) + 1) * OPTIM_CHUNK


def grad_pack(rows, n_rows, n_blocks, bucket, side=None, stream=None):
    """Every gradient of the table into its slot of ``bucket`` (float32 CUDA, >= grad_bucket_floats(n_blocks)), zeros behind each
    tensor; ``side`` (float32 CUDA, at most OPTIM_CHUNK values, or None) into the side chunk.  One launch (mnerf_grad_pack)."""
    lib = load()
    _f32c(bucket, "bucket")
    n_side = 0
    if side is not None:
        _f32c(side, "side")
        n_side = side.numel()
    if rows.numel() < n_rows * C.sizeof(OptimRow) or bucket.numel() < grad_bucket_floats(n_blocks) or n_side > OPTIM_CHUNK:
        raise MnerfError("grad_pack: rows / bucket too small for the table, or more than OPTIM_CHUNK side values")
    with _on(rows.device, stream) as st:
        check(lib.mnerf_grad_pack(_ptr(rows), int(n_rows), int(n_blocks), _ptr(side), n_side, _ptr(bucket), st), "mnerf_grad_pack")
    return bucket


def grad_unpack(rows, n_rows, n_blocks, bucket, scale, side_out=None, stream=None):
    """grad = bucket * scale for every row of the table, ``side_out`` (float32 CUDA or None) = the side slots * scale.  One launch
    (mnerf_grad_unpack); ``scale`` is rounded to fp32 on the way in."""
    lib = load()
    _f32c(bucket, "bucket")
    n_side = 0
    if side_out is not None:
        _f32c(side_out, "side_out")
        n_side = side_out.numel()
    if rows.numel() < n_rows * C.sizeof(OptimRow) or bucket.numel() < grad_bucket_floats(n_blocks) or n_side > OPTIM_CHUNK:
        raise MnerfError("grad_unpack: rows / bucket too small for the table, or more than OPTIM_CHUNK side values")
    with _on(rows.device, stream) as st:
        check(lib.mnerf_grad_unpack(_ptr(rows), int(n_rows), int(n_blocks), _ptr(bucket), float(scale), _ptr(side_out), n_side, st),
              "mnerf_grad_unpack")
    return side_out


# ----------------------------------------------------------------------- evaluation on the device (csrc/metrics.hip)


def image_metrics(pred, gt, invalid_mask=None, stream=None):
    """PSNR / SSIM of a batch of frames as ``metrics.psnr`` and ``metrics.EvalTools`` + ``metrics.ssim`` define them, on the device
    (mnerf_image_metrics; two launches, deterministic, fp64 arithmetic).  ``pred`` [B, H*W, 3] contiguous float32 CUDA (the rgb of
    a forward pass), ``gt`` [B, 3, H, W] float32 CUDA with contiguous images and any batch stride (``images[:, -1]`` passes without a
    copy), ``invalid_mask`` [B, H, W] bool / uint8 (non-zero = the pixel is dropped) or None for the 80 % centre crop.
    -> float64 CUDA tensor [B, 4]: PSNR in dB, SSIM, MSE, kept pixels.  Everything is checked here, before any launch."""
    import torch
    lib = load()
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise MnerfError(f"image_metrics: {name} must be a CUDA tensor, got {getattr(t, 'device', type(t))} (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise MnerfError(f"image_metrics: {name} must be float32, got {t.dtype}")
    if gt.dim() != 4 or gt.shape[1] != 3:
        raise MnerfError(f"image_metrics: gt must be [B, 3, H, W], got {tuple(gt.shape)}")
    b, _, h, w = gt.shape
    if tuple(pred.shape) != (b, h * w, 3) or pred.device != gt.device:
        raise MnerfError(f"image_metrics: pred {tuple(pred.shape)} on {pred.device} does not match gt {tuple(gt.shape)} on {gt.device}: "
                         f"expected [{b}, {h * w}, 3]")
    if not pred.is_contiguous():
        raise MnerfError("image_metrics: pred must be contiguous")
    if b < 1 or b > 65535:
        raise MnerfError(f"image_metrics: {b} images, the kernel takes 1..65535")
    if gt.stride()[1:] != (h * w, w, 1):
        raise MnerfError(f"image_metrics: every image of gt must be contiguous, got strides {gt.stride()}")
    gt_stride = gt.stride(0) if b > 1 else 3 * h * w
    if gt_stride < 3 * h * w:
        raise MnerfError(f"image_metrics: gt's images overlap (batch stride {gt_stride})")
    least = 10 if invalid_mask is None else 7
    if h < least or w < least:
        raise MnerfError(f"image_metrics: {h} x {w} images, the smallest is {least} x {least} "
                         + ("without a mask (the 80 % crop must hold a 7 x 7 window)" if invalid_mask is None else "with a mask (one 7 x 7 window)"))
    if invalid_mask is not None:
        if not torch.is_tensor(invalid_mask) or invalid_mask.device != pred.device or invalid_mask.dtype not in (torch.bool, torch.uint8):
            raise MnerfError("image_metrics: invalid_mask must be a bool or uint8 tensor on pred's device")
        if tuple(invalid_mask.shape) != (b, h, w):
            raise MnerfError(f"image_metrics: invalid_mask {tuple(invalid_mask.shape)}, expected [{b}, {h}, {w}]")
        invalid_mask = invalid_mask.contiguous()
        if invalid_mask.dtype == torch.bool:
            invalid_mask = invalid_mask.view(torch.uint8)  # one byte per element, 0 / 1
    n_bytes = lib.mnerf_image_metrics_workspace_bytes(b, h, w)
    if n_bytes <= 0:
        raise MnerfError(f"image_metrics: no workspace size for {b} images of {h} x {w}")
    with _on(pred.device, stream) as st:
        workspace = torch.empty(n_bytes // 8, dtype=torch.float64, device=pred.device)
        out = torch.empty((b, 4), dtype=torch.float64, device=pred.device)
        check(lib.mnerf_image_metrics(_ptr(pred), _ptr(gt), int(gt_stride), _ptr(invalid_mask), b, h, w, _ptr(workspace), _ptr(out), st),
              "mnerf_image_metrics")
        if stream is not None:  # the caching allocator must not hand the buffers on before this stream is through with them
            workspace.record_stream(stream)
            out.record_stream(stream)
    return out


# ----------------------------------------------------------------------- LPIPS on the device (csrc/lpips.hip)


def maxpool2x2(x, stream=None):
    """``F.max_pool2d(x, 2, 2)`` of a contiguous float32 CUDA tensor [..., H, W] -> [..., H // 2, W // 2] (mnerf_maxpool2x2)."""
    import torch
    lib = load()
    if not torch.is_tensor(x) or x.dim() < 2:
        raise MnerfError("maxpool2x2: expected a tensor [..., H, W]")
    _f32c(x, "x")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    planes = x.numel() // (h * w)
    out = torch.empty(tuple(x.shape[:-2]) + (h // 2, w // 2), dtype=torch.float32, device=x.device)
    with _on(x.device, stream) as st:
        check(lib.mnerf_maxpool2x2(_ptr(x), _ptr(out), planes, h, w, st), "mnerf_maxpool2x2")
    return out


def lpips_head(feat_a, feat_b, head_w, stream=None):
    """One stage of the LPIPS distance of one pair: feat_a, feat_b [C, H, W] float32 CUDA, head_w [C] -> float64 CUDA tensor [1]:
    mean over pixels of sum_c head_w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, all in fp64 (mnerf_lpips_head + mnerf_lpips_sum)."""
    import torch
    lib = load()
    for name, t in (("feat_a", feat_a), ("feat_b", feat_b), ("head_w", head_w)):
        _f32c(t, name)
    if feat_a.dim() != 3 or feat_a.shape != feat_b.shape or head_w.numel() != feat_a.shape[0]:
        raise MnerfError(f"lpips_head: feat_a {tuple(feat_a.shape)}, feat_b {tuple(feat_b.shape)}, head_w {tuple(head_w.shape)}")
    c, h, w = (int(v) for v in feat_a.shape)
    n_slots = int(lib.mnerf_lpips_head_slots(h, w))
    with _on(feat_a.device, stream) as st:
        slots = torch.empty(n_slots, dtype=torch.float64, device=feat_a.device)
        out = torch.empty(1, dtype=torch.float64, device=feat_a.device)
        check(lib.mnerf_lpips_head(_ptr(feat_a), _ptr(feat_b), _ptr(head_w), c, h, w, _ptr(slots), st), "mnerf_lpips_head")
        check(lib.mnerf_lpips_sum(_ptr(slots), n_slots, n_slots, 1, _ptr(out), st), "mnerf_lpips_sum")
        if stream is not None:
            slots.record_stream(stream)
            out.record_stream(stream)
    return out


class LpipsWeights:
    """The device-resident weights of ``lpips_vgg``: 13 x (wstream, bias, ew) in network order and the 5 head vectors, with the
    by-pointer table ``mnerf_lpips_vgg`` takes.  ``layers``: 13 (wstream float32 numpy / tensor from gmflow.pack_conv_blocks, bias
    [c_out], ew); ``heads``: 5 vectors.  (metrics.DeviceLPIPS builds one from the two weight files.)"""

    def __init__(self, layers, heads, device):
        import torch
        lib = load()
        if len(layers) != LPIPS_LAYERS or len(heads) != LPIPS_STAGES:
            raise MnerfError(f"LpipsWeights: {len(layers)} layers and {len(heads)} heads, expected {LPIPS_LAYERS} and {LPIPS_STAGES}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise MnerfError(f"LpipsWeights: the HIP kernels need a CUDA device, got {self.device} (there is no CPU fallback)")
        if self.device.index is None:  # "cuda": the current device, by its index (tensors report theirs)
            self.device = _current_device()
        to_dev = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not torch.is_tensor(a) else a.detach().float()).contiguous().to(self.device)
        self.table = LpipsWeightTable()
        self.tensors = []
        for l, (ws, bias, ew) in enumerate(layers):
            ws, bias = to_dev(ws).reshape(-1), to_dev(bias).reshape(-1)
            if ws.numel() != lib.mnerf_lpips_wstream_floats(l):
                raise MnerfError(f"LpipsWeights: layer {l} has a stream of {ws.numel()} words, expected {lib.mnerf_lpips_wstream_floats(l)}")
            self.tensors += [ws, bias]
            self.table.wstream[l], self.table.bias[l], self.table.ew[l] = ws.data_ptr(), bias.data_ptr(), int(ew)
        for l, hw in enumerate(heads):
            hw = to_dev(hw).reshape(-1)
            self.tensors.append(hw)
            self.table.head[l] = hw.data_ptr()


def lpips_workspace_bytes(n_images, height, width, masked):
    """bytes of the workspace of ``lpips_vgg`` (mnerf_lpips_workspace_bytes; -1: no image, or a processed image below 16 x 16)"""
    return int(load().mnerf_lpips_workspace_bytes(int(n_images), int(height), int(width), int(bool(masked))))


def lpips_vgg(pred, gt, invalid_mask, weights, workspace=None, stream=None):
    """LPIPS (VGG-16 variant, ``metrics.LPIPSVGG``) of a batch of frames on the device (mnerf_lpips_vgg): ``pred`` [B, H*W, 3], ``gt``
    [B, 3, H, W], ``invalid_mask`` [B, H, W] bool / uint8 or None - exactly the arguments of ``image_metrics`` -, ``weights`` an
    ``LpipsWeights``.  With a mask the masked pixels are zeroed in both images, without one the 80 % centre crop is scored.
    -> float64 CUDA tensor [B].  ``workspace``: a uint8 CUDA tensor of at least ``lpips_workspace_bytes`` bytes to reuse, or None.
    Everything is checked here, before any launch; CPU tensors raise (there is no CPU fallback)."""
    import torch
    lib = load()
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise MnerfError(f"lpips_vgg: {name} must be a CUDA tensor, got {getattr(t, 'device', type(t))} (there is no CPU fallback)")
        if t.dtype != torch.float32:
            raise MnerfError(f"lpips_vgg: {name} must be float32, got {t.dtype}")
    if not isinstance(weights, LpipsWeights) or weights.device != pred.device:
        raise MnerfError(f"lpips_vgg: weights must be an LpipsWeights on {pred.device}")
    if gt.dim() != 4 or gt.shape[1] != 3:
        raise MnerfError(f"lpips_vgg: gt must be [B, 3, H, W], got {tuple(gt.shape)}")
    b, _, h, w = gt.shape
    if tuple(pred.shape) != (b, h * w, 3) or pred.device != gt.device:
        raise MnerfError(f"lpips_vgg: pred {tuple(pred.shape)} on {pred.device} does not match gt {tuple(gt.shape)} on {gt.device}: "
                         f"expected [{b}, {h * w}, 3]")
    if not pred.is_contiguous():
        raise MnerfError("lpips_vgg: pred must be contiguous")
    if b < 1 or b > 65535:
        raise MnerfError(f"lpips_vgg: {b} images, the kernel takes 1..65535")
    if gt.stride()[1:] != (h * w, w, 1):
        raise MnerfError(f"lpips_vgg: every image of gt must be contiguous, got strides {gt.stride()}")
    gt_stride = gt.stride(0) if b > 1 else 3 * h * w
    if gt_stride < 3 * h * w:
        raise MnerfError(f"lpips_vgg: gt's images overlap (batch stride {gt_stride})")
    if invalid_mask is not None:
        if not torch.is_tensor(invalid_mask) or invalid_mask.device != pred.device or invalid_mask.dtype not in (torch.bool, torch.uint8):
            raise MnerfError("lpips_vgg: invalid_mask must be a bool or uint8 tensor on pred's device")
        if tuple(invalid_mask.shape) != (b, h, w):
            raise MnerfError(f"lpips_vgg: invalid_mask {tuple(invalid_mask.shape)}, expected [{b}, {h}, {w}]")
        invalid_mask = invalid_mask.contiguous()
        if invalid_mask.dtype == torch.bool:
            invalid_mask = invalid_mask.view(torch.uint8)
    n_bytes = lib.mnerf_lpips_workspace_bytes(b, h, w, int(invalid_mask is not None))
    if n_bytes <= 0:
        raise MnerfError(f"lpips_vgg: {h} x {w} images: the processed image (the whole frame with a mask, the 80 % centre crop without) "
                         "must be at least 16 x 16")
    if workspace is not None and (not torch.is_tensor(workspace) or workspace.device != pred.device or workspace.dtype != torch.uint8
                                  or not workspace.is_contiguous() or workspace.numel() < n_bytes):
        raise MnerfError(f"lpips_vgg: workspace must be a contiguous uint8 tensor of at least {n_bytes} bytes on {pred.device}")
    with _on(pred.device, stream) as st:
        if workspace is None:
            workspace = torch.empty(n_bytes, dtype=torch.uint8, device=pred.device)
        out = torch.empty(b, dtype=torch.float64, device=pred.device)
        check(lib.mnerf_lpips_vgg(_ptr(pred), _ptr(gt), int(gt_stride), _ptr(invalid_mask), b, h, w, C.byref(weights.table),
                                  _ptr(workspace), _ptr(out), st), "mnerf_lpips_vgg")
        if stream is not None:
            workspace.record_stream(stream)
            out.record_stream(stream)
    return out


# ----------------------------------------------------------------------- geometry export (matchnerf_amd/csrc/fusion.hip)

POINT_FLOATS = 8  # floats of one row of a point buffer: x y z d | r g b n


def view_array(views):
    """[View, ...] -> a host array of mnerf_view, as mnerf_depth_consistency reads it during the call"""
    arr = (View * len(views))()
    for i, v in enumerate(views):
        arr[i] = v
    return arr


def depth_consistency(views, ref, depth, opacity=None, legacy=True, px_tol=1.0, rel_tol=0.01, min_opacity=0.5, out=None, stream=None):
    """Cross-view consistency of view ``ref``'s depth map against the other views' (mnerf_depth_consistency; the criterion is stated
    in include/mnerf.h).  ``views``: a list of View - extr, the intr of the maps' grid, near_ / far_ = the valid depth range;
    ``depth`` [K, h, w] float32 CUDA camera-z depths; ``opacity`` the same shape or None.  -> (fused_depth [h, w] float32,
    n_consistent [h, w] int32), or the pair ``out`` filled."""
    import torch
    lib = load()
    _f32c(depth, "depth")
    if depth.dim() != 3 or depth.shape[0] != len(views):
        raise MnerfError(f"depth_consistency: depth {tuple(depth.shape)} is not [{len(views)}, h, w]")
    if opacity is not None and (_f32c(opacity, "opacity").shape != depth.shape or opacity.device != depth.device):
        raise MnerfError(f"depth_consistency: opacity {tuple(opacity.shape)} on {opacity.device} does not match depth {tuple(depth.shape)}")
    k, h, w = (int(x) for x in depth.shape)
    if out is None:
        out = (torch.empty(h, w, device=depth.device), torch.empty(h, w, dtype=torch.int32, device=depth.device))
    fused, cnt = out
    if _f32c(fused, "fused_depth").numel() != h * w or cnt.dtype != torch.int32 or cnt.numel() != h * w or not cnt.is_contiguous() \
            or fused.device != depth.device or cnt.device != depth.device:
        raise MnerfError(f"depth_consistency: out must be (float32, int32) of {h * w} elements on {depth.device}")
    arr = views if isinstance(views, C.Array) else view_array(views)
    with _on(depth.device, stream) as st:
        check(lib.mnerf_depth_consistency(arr, k, int(ref), h, w, int(bool(legacy)), _ptr(depth), _ptr(opacity), float(px_tol),
                                          float(rel_tol), float(min_opacity), _ptr(fused), _ptr_i32(cnt), st), "mnerf_depth_consistency")
    return fused, cnt


def export_workspace(what, workspace, need, dev):
    """the workspace of an export call: the caller's if it lies on ``dev`` and holds ``need`` bytes, a fresh one for None"""
    import torch
    if workspace is None:
        return torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if workspace.device != dev or workspace.numel() * workspace.element_size() < need:
        raise MnerfError(f"{what}: workspace of {workspace.numel() * workspace.element_size()} bytes on {workspace.device}, "
                         f"{need} needed on {dev}")
    return workspace


def point_cloud_workspace_bytes(n_pixels):
    return int(load().mnerf_point_cloud_workspace_bytes(int(n_pixels)))


def point_cloud(view, hw, depth, rgb, n_consistent, min_consistent, legacy=True, points=None, count=None, workspace=None,
                stream=None):
    """The selected pixels of one view as rows ``x y z d | r g b n`` in pixel order (mnerf_point_cloud: a stable compaction, no atomic
    cursor).  ``depth`` [h*w] float32 CUDA (the fused depth), ``rgb`` [h*w, 3], ``n_consistent`` [h*w] int32.  ``points``
    [capacity, 8] float32 (default: h*w rows), ``count`` a 1-element int64 tensor, ``workspace`` a uint8 tensor of
    ``point_cloud_workspace_bytes(h*w)`` bytes - allocated when None.  Enqueue only: -> (points, count); rows at or beyond the
    capacity are not written, ``count`` is the total either way."""
    import torch
    lib = load()
    h, w = int(hw[0]), int(hw[1])
    n = h * w
    dev = depth.device
    _f32c(depth, "depth"), _f32c(rgb, "rgb")
    if depth.numel() != n or rgb.numel() != 3 * n or rgb.device != dev:
        raise MnerfError(f"point_cloud: depth {tuple(depth.shape)} / rgb {tuple(rgb.shape)} are not [{n}] / [{n}, 3] on one device")
    if n_consistent.dtype != torch.int32 or n_consistent.numel() != n or not n_consistent.is_contiguous() or n_consistent.device != dev:
        raise MnerfError(f"point_cloud: n_consistent must be a contiguous int32 tensor of {n} elements on {dev}")
    if points is None:
        points = torch.empty(n, POINT_FLOATS, device=dev)
    if _f32c(points, "points").device != dev or points.numel() % POINT_FLOATS:
        raise MnerfError(f"point_cloud: points {tuple(points.shape)} on {points.device} is no [capacity, {POINT_FLOATS}] buffer on {dev}")
    count = torch.zeros(1, dtype=torch.int64, device=dev) if count is None else _mesh_buffer("point_cloud", "count", count, torch.int64, 1, dev)
    workspace = export_workspace("point_cloud", workspace, point_cloud_workspace_bytes(n), dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_point_cloud(C.byref(view), h, w, int(bool(legacy)), _ptr(depth), _ptr(rgb), _ptr_i32(n_consistent),
                                    int(min_consistent), _ptr(points), points.numel() // POINT_FLOATS, _ptr(count), _ptr(workspace), st),
              "mnerf_point_cloud")
    return points, count


def depth_colormap(depth, lo, hi, out=None, stream=None):
    """Depth values -> JET colours, uint8 [..., 3] (mnerf_depth_colormap: the arithmetic of the reference's visualize_depth with the
    index clamped and the map stated as a formula, include/mnerf.h)."""
    import torch
    lib = load()
    _f32c(depth, "depth")
    if out is None:
        out = torch.empty(tuple(depth.shape) + (3,), dtype=torch.uint8, device=depth.device)
    if out.dtype != torch.uint8 or out.numel() != 3 * depth.numel() or not out.is_contiguous() or out.device != depth.device:
        raise MnerfError(f"depth_colormap: out must be a contiguous uint8 tensor of {3 * depth.numel()} elements on {depth.device}")
    with _on(depth.device, stream) as st:
        check(lib.mnerf_depth_colormap(_ptr(depth), depth.numel(), float(lo), float(hi), _ptr(out), st), "mnerf_depth_colormap")
    return out


# ----------------------------------------------------------------------- mesh export (matchnerf_amd/csrc/mesh.hip)

VERTEX_FLOATS = 8  # floats of one row of a vertex buffer: x y z w | r g b 0


def _grid(origin, voxel, dims):
    """(origin xyz, voxel, (nx, ny, nz)) -> the seven scalars of the header's grid"""
    if len(origin) != 3 or len(dims) != 3:
        raise MnerfError(f"a grid is an origin of 3 floats and (nx, ny, nz), got {origin!r} / {dims!r}")
    return [float(x) for x in origin] + [float(voxel)] + [int(x) for x in dims]


def tsdf_integrate(views, depth, rgb, origin, voxel, dims, trunc, sums, weight, opacity=None, n_consistent=None, min_consistent=0,
                   legacy=True, min_opacity=0.5, stream=None):
    """Add the depth maps of up to MNERF_MAX_VIEWS views to a TSDF volume (mnerf_tsdf_integrate; the update is stated in
    include/mnerf.h).  ``views``: a list of View as for ``depth_consistency``; ``depth`` [K, h, w] float32 CUDA, ``opacity`` the same
    shape or None, ``rgb`` [K, h*w, 3]; ``n_consistent`` [K, h, w] int32 or None - with it ``depth`` is the fused depth and a texel
    needs ``n_consistent >= min_consistent``.  The grid: ``origin`` (x, y, z), ``voxel``, ``dims`` = (nx, ny, nz).  ``sums``
    [nz, ny, nx, 4] and ``weight`` [nz, ny, nx] float32 are the caller's, zeroed before the first call; calls accumulate.
    Enqueue only: -> (sums, weight)."""
    import torch
    lib = load()
    _f32c(depth, "depth"), _f32c(rgb, "rgb"), _f32c(sums, "sums"), _f32c(weight, "weight")
    dev = depth.device
    if depth.dim() != 3 or depth.shape[0] != len(views):
        raise MnerfError(f"tsdf_integrate: depth {tuple(depth.shape)} is not [{len(views)}, h, w]")
    k, h, w = (int(x) for x in depth.shape)
    if rgb.numel() != 3 * depth.numel() or rgb.device != dev:
        raise MnerfError(f"tsdf_integrate: rgb {tuple(rgb.shape)} on {rgb.device} is not [{k}, {h * w}, 3] on {dev}")
    if opacity is not None and (_f32c(opacity, "opacity").shape != depth.shape or opacity.device != dev):
        raise MnerfError(f"tsdf_integrate: opacity {tuple(opacity.shape)} on {opacity.device} does not match depth {tuple(depth.shape)}")
    if n_consistent is not None and (n_consistent.dtype != torch.int32 or n_consistent.numel() != depth.numel()
                                     or not n_consistent.is_contiguous() or n_consistent.device != dev):
        raise MnerfError(f"tsdf_integrate: n_consistent must be a contiguous int32 tensor of {depth.numel()} elements on {dev}")
    grid = _grid(origin, voxel, dims)
    n = grid[4] * grid[5] * grid[6]
    if sums.numel() != 4 * n or weight.numel() != n or sums.device != dev or weight.device != dev:
        raise MnerfError(f"tsdf_integrate: sums {tuple(sums.shape)} / weight {tuple(weight.shape)} are not [nz, ny, nx, 4] / "
                         f"[nz, ny, nx] of the grid {tuple(grid[4:])} on {dev}")
    arr = views if isinstance(views, C.Array) else view_array(views)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_integrate(arr, k, h, w, int(bool(legacy)), _ptr(depth), _ptr(opacity), _ptr_i32(n_consistent),
                                       int(min_consistent), _ptr(rgb), float(min_opacity), float(trunc), *grid, _ptr(sums), _ptr(weight),
                                       st), "mnerf_tsdf_integrate")
    return sums, weight


def tsdf_mesh_workspace_bytes(dims):
    return int(load().mnerf_tsdf_mesh_workspace_bytes(int(dims[0]), int(dims[1]), int(dims[2])))


def tsdf_mesh(sums, weight, origin, voxel, dims, min_weight, vertices, triangles, counts=None, workspace=None, stream=None):
    """The triangle mesh of a TSDF volume (mnerf_tsdf_mesh: marching tetrahedra, welded vertices, a defined order and no atomics).
    ``vertices`` [vertex capacity, 8] float32 rows ``x y z w | r g b 0``, ``triangles`` [triangle capacity, 3] int32, ``counts`` a
    2-element int64 tensor (vertices, triangles), ``workspace`` a uint8 tensor of ``tsdf_mesh_workspace_bytes(dims)`` bytes - the last
    two allocated when None.  Enqueue only: -> (vertices, triangles, counts); rows at or beyond a capacity are not written, the
    counts are the totals either way."""
    import torch
    lib = load()
    _f32c(sums, "sums"), _f32c(weight, "weight"), _f32c(vertices, "vertices")
    dev = sums.device
    grid = _grid(origin, voxel, dims)
    n = grid[4] * grid[5] * grid[6]
    if sums.numel() != 4 * n or weight.numel() != n or weight.device != dev:
        raise MnerfError(f"tsdf_mesh: sums {tuple(sums.shape)} / weight {tuple(weight.shape)} are not [nz, ny, nx, 4] / [nz, ny, nx] "
                         f"of the grid {tuple(grid[4:])} on {dev}")
    if vertices.device != dev or vertices.numel() % VERTEX_FLOATS:
        raise MnerfError(f"tsdf_mesh: vertices {tuple(vertices.shape)} on {vertices.device} is no [capacity, {VERTEX_FLOATS}] buffer on {dev}")
    if triangles.dtype != torch.int32 or not triangles.is_contiguous() or triangles.device != dev or triangles.numel() % 3:
        raise MnerfError(f"tsdf_mesh: triangles must be a contiguous int32 [capacity, 3] tensor on {dev}")
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else _mesh_buffer("tsdf_mesh", "counts", counts, torch.int64, 2, dev)
    need = tsdf_mesh_workspace_bytes(grid[4:])
    if need < 0:
        raise MnerfError(f"tsdf_mesh: the grid {tuple(grid[4:])} is too large to mesh")
    workspace = export_workspace("tsdf_mesh", workspace, need, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_mesh(_ptr(sums), _ptr(weight), *grid, float(min_weight), _ptr(vertices), vertices.numel() // VERTEX_FLOATS,
                                  _ptr_i32(triangles), triangles.numel() // 3, _ptr(counts), _ptr(workspace), st), "mnerf_tsdf_mesh")
    return vertices, triangles, counts


# ----------------------------------------------------------------------- sparse TSDF volume (matchnerf_amd/csrc/tsdf_sparse.hip)

TSDF_BRICK = 8  # MNERF_TSDF_BRICK: voxels per side of a brick
BRICK_POINTS = TSDF_BRICK ** 3
MAX_BRICKS = ((1 << 31) - 1) // 12 // BRICK_POINTS  # what mnerf_tsdf_mesh_sparse takes: 349 525


def brick_dims(dims):
    """(nx, ny, nz) -> (bx, by, bz), the bricks that cover the virtual grid"""
    return tuple(-(-int(d) // TSDF_BRICK) for d in dims)


def _sparse_maps(what, views, depth, opacity, n_consistent):
    """the checks of ``tsdf_integrate`` on the maps -> (device, K, h, w)"""
    import torch
    _f32c(depth, "depth")
    dev = depth.device
    if depth.dim() != 3 or depth.shape[0] != len(views):
        raise MnerfError(f"{what}: depth {tuple(depth.shape)} is not [{len(views)}, h, w]")
    if opacity is not None and (_f32c(opacity, "opacity").shape != depth.shape or opacity.device != dev):
        raise MnerfError(f"{what}: opacity {tuple(opacity.shape)} on {opacity.device} does not match depth {tuple(depth.shape)}")
    if n_consistent is not None and (n_consistent.dtype != torch.int32 or n_consistent.numel() != depth.numel()
                                     or not n_consistent.is_contiguous() or n_consistent.device != dev):
        raise MnerfError(f"{what}: n_consistent must be a contiguous int32 tensor of {depth.numel()} elements on {dev}")
    return (dev,) + tuple(int(x) for x in depth.shape)


def _brick_tables(what, grid, table, bricks, n_bricks, dev):
    """``table`` / ``bricks`` of the grid's bricks and ``n_bricks`` within them -> the number of bricks of the virtual grid"""
    import torch
    bx, by, bz = brick_dims(grid[4:])
    for name, t in (("table", table), ("bricks", bricks)):
        if t is not None:
            _mesh_buffer(what, name, t, torch.int32, bx * by * bz, dev)
    if not 0 <= int(n_bricks) <= bx * by * bz:
        raise MnerfError(f"{what}: n_bricks={n_bricks} outside 0..{bx * by * bz}, the bricks of the grid {tuple(grid[4:])}")
    return bx * by * bz


def tsdf_bricks_mark(views, depth, origin, voxel, dims, trunc, marks, opacity=None, n_consistent=None, min_consistent=0, legacy=True,
                     min_opacity=0.5, stream=None):
    """Mark the 8^3-voxel bricks of the virtual grid that a surface of the maps can touch (mnerf_tsdf_bricks_mark; the rule is stated
    in include/mnerf.h).  Maps and grid as for ``tsdf_integrate``; ``marks`` uint8 [bz, by, bx] (``brick_dims(dims)``) is the
    caller's, zeroed before the first call; calls OR into it.  Enqueue only: -> marks."""
    import torch
    lib = load()
    dev, k, h, w = _sparse_maps("tsdf_bricks_mark", views, depth, opacity, n_consistent)
    grid = _grid(origin, voxel, dims)
    bx, by, bz = brick_dims(grid[4:])
    _mesh_buffer("tsdf_bricks_mark", "marks", marks, torch.uint8, bx * by * bz, dev)
    arr = views if isinstance(views, C.Array) else view_array(views)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_bricks_mark(arr, k, h, w, int(bool(legacy)), _ptr(depth), _ptr(opacity), _ptr_i32(n_consistent),
                                         int(min_consistent), float(min_opacity), float(trunc), *grid, _ptr(marks), st),
              "mnerf_tsdf_bricks_mark")
    return marks


def tsdf_bricks_table_workspace_bytes(bdims):
    return int(load().mnerf_tsdf_bricks_table_workspace_bytes(int(bdims[0]), int(bdims[1]), int(bdims[2])))


def tsdf_bricks_table(marks, bdims, table=None, bricks=None, count=None, workspace=None, stream=None):
    """Marks -> (table int32 [bz, by, bx]: every marked brick's slot, ascending with its linear index, -1 elsewhere; bricks int32
    [bx by bz]: the marked bricks' linear indices in its first ``count`` entries; count: a 1-element int64 tensor) on the device
    (mnerf_tsdf_bricks_table).  ``bdims`` = (bx, by, bz).  Enqueue only: the caller copies the count."""
    import torch
    lib = load()
    bx, by, bz = (int(b) for b in bdims)
    dev = marks.device
    need = tsdf_bricks_table_workspace_bytes((bx, by, bz))
    if need < 0:
        raise MnerfError(f"tsdf_bricks_table: {bx}x{by}x{bz} bricks are out of range")
    n = bx * by * bz
    _mesh_buffer("tsdf_bricks_table", "marks", marks, torch.uint8, n, dev)
    table = _mesh_buffer("tsdf_bricks_table", "table", table, torch.int32, n, dev).view(bz, by, bx)
    bricks = _mesh_buffer("tsdf_bricks_table", "bricks", bricks, torch.int32, n, dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev) if count is None else _mesh_buffer("tsdf_bricks_table", "count", count, torch.int64, 1, dev)
    workspace = export_workspace("tsdf_bricks_table", workspace, need, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_bricks_table(_ptr(marks), bx, by, bz, _ptr_i32(table), _ptr_i32(bricks), _ptr(count), _ptr(workspace), st),
              "mnerf_tsdf_bricks_table")
    return table, bricks, count


def tsdf_integrate_sparse(views, depth, rgb, origin, voxel, dims, trunc, bricks, n_bricks, sums, weight, opacity=None, n_consistent=None,
                          min_consistent=0, legacy=True, min_opacity=0.5, stream=None):
    """``tsdf_integrate`` on the allocated bricks of a sparse volume (mnerf_tsdf_integrate_sparse): ``bricks`` and ``n_bricks`` from
    ``tsdf_bricks_table``; ``sums`` [n_bricks, 512, 4] and ``weight`` [n_bricks, 512] float32 are the caller's, zeroed before the
    first call; calls accumulate.  Every allocated voxel gets the bits of the dense volume.  Enqueue only: -> (sums, weight)."""
    lib = load()
    what = "tsdf_integrate_sparse"
    dev, k, h, w = _sparse_maps(what, views, depth, opacity, n_consistent)
    _f32c(rgb, "rgb"), _f32c(sums, "sums"), _f32c(weight, "weight")
    if rgb.numel() != 3 * depth.numel() or rgb.device != dev:
        raise MnerfError(f"{what}: rgb {tuple(rgb.shape)} on {rgb.device} is not [{k}, {h * w}, 3] on {dev}")
    grid = _grid(origin, voxel, dims)
    n_bricks = int(n_bricks)
    _brick_tables(what, grid, None, bricks, n_bricks, dev)
    if sums.numel() != 4 * BRICK_POINTS * n_bricks or weight.numel() != BRICK_POINTS * n_bricks or sums.device != dev or weight.device != dev:
        raise MnerfError(f"{what}: sums {tuple(sums.shape)} / weight {tuple(weight.shape)} are not [{n_bricks}, {BRICK_POINTS}, 4] / "
                         f"[{n_bricks}, {BRICK_POINTS}] on {dev}")
    arr = views if isinstance(views, C.Array) else view_array(views)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_integrate_sparse(arr, k, h, w, int(bool(legacy)), _ptr(depth), _ptr(opacity), _ptr_i32(n_consistent),
                                              int(min_consistent), _ptr(rgb), float(min_opacity), float(trunc), *grid, _ptr_i32(bricks),
                                              n_bricks, _ptr(sums), _ptr(weight), st), "mnerf_tsdf_integrate_sparse")
    return sums, weight


def tsdf_mesh_sparse_workspace_bytes(n_bricks, bdims):
    return int(load().mnerf_tsdf_mesh_sparse_workspace_bytes(int(n_bricks), int(bdims[0]), int(bdims[1]), int(bdims[2])))


def tsdf_mesh_sparse(sums, weight, table, bricks, n_bricks, origin, voxel, dims, min_weight, vertices, triangles, counts=None,
                     workspace=None, stream=None):
    """The triangle mesh of a sparse TSDF volume (mnerf_tsdf_mesh_sparse): the mesh of ``tsdf_mesh`` on the dense volume, bit for
    bit, with the vertices in the order (slot, in-brick index, direction) and the triangles in (slot, in-brick index, tet, triangle).
    Volume and tables as for ``tsdf_integrate_sparse``; the other arguments as for ``tsdf_mesh``, ``workspace`` of
    ``tsdf_mesh_sparse_workspace_bytes(n_bricks, brick_dims(dims))`` bytes.  Enqueue only: -> (vertices, triangles, counts)."""
    import torch
    lib = load()
    what = "tsdf_mesh_sparse"
    _f32c(sums, "sums"), _f32c(weight, "weight"), _f32c(vertices, "vertices")
    dev = sums.device
    grid = _grid(origin, voxel, dims)
    n_bricks = int(n_bricks)
    _brick_tables(what, grid, table, bricks, n_bricks, dev)
    if sums.numel() != 4 * BRICK_POINTS * n_bricks or weight.numel() != BRICK_POINTS * n_bricks or weight.device != dev:
        raise MnerfError(f"{what}: sums {tuple(sums.shape)} / weight {tuple(weight.shape)} are not [{n_bricks}, {BRICK_POINTS}, 4] / "
                         f"[{n_bricks}, {BRICK_POINTS}] on {dev}")
    if vertices.device != dev or vertices.numel() % VERTEX_FLOATS:
        raise MnerfError(f"{what}: vertices {tuple(vertices.shape)} on {vertices.device} is no [capacity, {VERTEX_FLOATS}] buffer on {dev}")
    if triangles.dtype != torch.int32 or not triangles.is_contiguous() or triangles.device != dev or triangles.numel() % 3:
        raise MnerfError(f"{what}: triangles must be a contiguous int32 [capacity, 3] tensor on {dev}")
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else _mesh_buffer(what, "counts", counts, torch.int64, 2, dev)
    need = tsdf_mesh_sparse_workspace_bytes(n_bricks, brick_dims(grid[4:]))
    if need < 0:
        raise MnerfError(f"{what}: {n_bricks} bricks of the grid {tuple(grid[4:])} are too many to mesh (at most {MAX_BRICKS})")
    workspace = export_workspace(what, workspace, need, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_tsdf_mesh_sparse(_ptr(sums), _ptr(weight), _ptr_i32(table), _ptr_i32(bricks), n_bricks, *grid, float(min_weight),
                                         _ptr(vertices), vertices.numel() // VERTEX_FLOATS, _ptr_i32(triangles), triangles.numel() // 3,
                                         _ptr(counts), _ptr(workspace), st), "mnerf_tsdf_mesh_sparse")
    return vertices, triangles, counts


# ----------------------------------------------------------------------- mesh finishing (matchnerf_amd/csrc/mesh_finish.hip)

NORMAL_FLOATS = 4  # floats of one row of a normal buffer: nx ny nz a
VERTEX_BOUNDARY, VERTEX_INTERIOR = 0, 1  # the class bytes of mesh_adjacency


def mesh_finish_workspace_bytes(n_vertices, n_triangles):
    return int(load().mnerf_mesh_finish_workspace_bytes(int(n_vertices), int(n_triangles)))


def _mesh_args(what, vertices, triangles, n_vertices=None):
    """the checks of ``tsdf_mesh`` on an indexed mesh -> (device, V, T); ``vertices`` None: a function that takes the faces alone"""
    import torch
    if triangles.dtype != torch.int32 or not triangles.is_contiguous() or not triangles.is_cuda or triangles.numel() % 3:
        raise MnerfError(f"{what}: triangles must be a contiguous int32 [T, 3] CUDA tensor, got {triangles.dtype} "
                         f"{tuple(triangles.shape)} on {triangles.device}")
    dev = triangles.device
    if vertices is not None:
        _f32c(vertices, "vertices")
        if vertices.device != dev or vertices.numel() % VERTEX_FLOATS:
            raise MnerfError(f"{what}: vertices {tuple(vertices.shape)} on {vertices.device} is no [V, {VERTEX_FLOATS}] buffer on {dev}")
        n_vertices = vertices.numel() // VERTEX_FLOATS
    n_vertices = int(n_vertices)
    if mesh_finish_workspace_bytes(n_vertices, triangles.numel() // 3) < 0:
        raise MnerfError(f"{what}: {n_vertices} vertices / {triangles.numel() // 3} triangles are out of range")
    return dev, n_vertices, triangles.numel() // 3


def _mesh_buffer(what, name, t, dtype, numel, dev):
    """an output or table the caller passes, or a fresh one"""
    import torch
    if t is None:
        return torch.empty(numel, dtype=dtype, device=dev)
    if t.dtype != dtype or t.numel() != numel or t.device != dev or not t.is_contiguous():
        raise MnerfError(f"{what}: {name} must be a contiguous {dtype} tensor of {numel} elements on {dev}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def _mesh_workspace(what, workspace, n_vertices, n_triangles, dev):
    return export_workspace(what, workspace, mesh_finish_workspace_bytes(n_vertices, n_triangles), dev)


def mesh_adjacency(triangles, n_vertices, out=None, workspace=None, stream=None):
    """The vertex -> corner table of an indexed mesh (mnerf_mesh_adjacency): ``triangles`` [T, 3] int32 CUDA over ``n_vertices``
    vertices -> (offsets int32 [V + 1], corners int32 [3 T], vertex_class uint8 [V]): row v = corners[offsets[v]:offsets[v + 1]]
    lists ascending the corners 3 t + k with triangles[t, k] == v; the class is VERTEX_INTERIOR or VERTEX_BOUNDARY.  ``out``: the
    three tensors to write into.  Enqueue only."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_adjacency", None, triangles, n_vertices)
    workspace = _mesh_workspace("mesh_adjacency", workspace, nv, nt, dev)
    out = (None, None, None) if out is None else out
    offsets = _mesh_buffer("mesh_adjacency", "offsets", out[0], torch.int32, nv + 1, dev)
    corners = _mesh_buffer("mesh_adjacency", "corners", out[1], torch.int32, 3 * nt, dev)
    vclass = _mesh_buffer("mesh_adjacency", "vertex_class", out[2], torch.uint8, nv, dev)
    if nv == 0:  # the library touches no buffer then
        offsets.zero_()
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_adjacency(_ptr_i32(triangles), nv, nt, _ptr_i32(offsets), _ptr_i32(corners), _ptr(vclass), _ptr(workspace), st),
              "mnerf_mesh_adjacency")
    return offsets, corners, vclass


def mesh_components(triangles, n_vertices, min_triangles=0, min_fraction=0.0, out=None, workspace=None, stream=None):
    """Connected components of an indexed mesh (mnerf_mesh_components) -> (labels int32 [V]: the smallest vertex row of the vertex's
    component, keep uint8 [V]: 1 iff the component has at least ``min_triangles`` triangles and at least ``min_fraction`` of the
    largest component's).  ``out``: the two tensors to write into.  Enqueue only, no copy."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_components", None, triangles, n_vertices)
    workspace = _mesh_workspace("mesh_components", workspace, nv, nt, dev)
    out = (None, None) if out is None else out
    labels = _mesh_buffer("mesh_components", "labels", out[0], torch.int32, nv, dev)
    keep = _mesh_buffer("mesh_components", "keep", out[1], torch.uint8, nv, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_components(_ptr_i32(triangles), nv, nt, int(min_triangles), float(min_fraction), _ptr_i32(labels), _ptr(keep),
                                        _ptr(workspace), st), "mnerf_mesh_components")
    return labels, keep


def mesh_compact(vertices, triangles, keep, vertices_out=None, triangles_out=None, counts=None, workspace=None, stream=None):
    """The mesh of the vertices whose ``keep`` byte is set (mnerf_mesh_compact): kept rows bit for bit and in order, a triangle kept
    iff its first vertex is, indices re-numbered.  ``vertices_out`` [capacity, 8] / ``triangles_out`` [capacity, 3] default to the
    input's sizes, ``counts`` is a 2-element int64 tensor.  Enqueue only: -> (vertices_out, triangles_out, counts); rows at or beyond
    a capacity are not written, the counts are the totals either way."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_compact", vertices, triangles)
    keep = _mesh_buffer("mesh_compact", "keep", keep, torch.uint8, nv, dev)
    if vertices_out is None:
        vertices_out = torch.empty(nv, VERTEX_FLOATS, device=dev)
    if triangles_out is None:
        triangles_out = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    _mesh_args("mesh_compact", vertices_out, triangles_out)
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else _mesh_buffer("mesh_compact", "counts", counts,
                                                                                              torch.int64, 2, dev)
    workspace = _mesh_workspace("mesh_compact", workspace, nv, nt, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_compact(_ptr(vertices), _ptr_i32(triangles), nv, nt, _ptr(keep), _ptr(vertices_out),
                                     vertices_out.numel() // VERTEX_FLOATS, _ptr_i32(triangles_out), triangles_out.numel() // 3,
                                     _ptr(counts), _ptr(workspace), st), "mnerf_mesh_compact")
    return vertices_out, triangles_out, counts


def mesh_smooth(vertices, triangles, adjacency, iterations, lam=0.5, mu=-0.53, out=None, workspace=None, stream=None):
    """``iterations`` rounds of Taubin smoothing of the positions (mnerf_mesh_smooth: p + lam L(p), then p + mu L(p), L the uniform
    umbrella on interior vertices; boundary vertices and the fields w | r g b 0 do not change).  ``adjacency`` = the triple of
    ``mesh_adjacency`` for this mesh.  ``out`` may be ``vertices`` (in place); default a new tensor.  Enqueue only: -> out."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_smooth", vertices, triangles)
    offsets = _mesh_buffer("mesh_smooth", "offsets", adjacency[0], torch.int32, nv + 1, dev)
    corners = _mesh_buffer("mesh_smooth", "corners", adjacency[1], torch.int32, 3 * nt, dev)
    vclass = _mesh_buffer("mesh_smooth", "vertex_class", adjacency[2], torch.uint8, nv, dev)
    out = _mesh_buffer("mesh_smooth", "out", out, torch.float32, nv * VERTEX_FLOATS, dev).view(nv, VERTEX_FLOATS)
    workspace = _mesh_workspace("mesh_smooth", workspace, nv, nt, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_smooth(_ptr(vertices), nv, _ptr_i32(triangles), nt, _ptr_i32(offsets), _ptr_i32(corners), _ptr(vclass),
                                    int(iterations), float(lam), float(mu), _ptr(out), _ptr(workspace), st), "mnerf_mesh_smooth")
    return out


def mesh_normals(vertices, triangles, adjacency, out=None, stream=None):
    """Area-weighted vertex normals (mnerf_mesh_normals) -> [V, 4] float32 rows ``nx ny nz a``: the normalised corner sum of the
    triangles' cross products (0 0 0 where it vanishes) and a third of the incident area.  ``adjacency`` as for ``mesh_smooth``."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_normals", vertices, triangles)
    offsets = _mesh_buffer("mesh_normals", "offsets", adjacency[0], torch.int32, nv + 1, dev)
    corners = _mesh_buffer("mesh_normals", "corners", adjacency[1], torch.int32, 3 * nt, dev)
    out = _mesh_buffer("mesh_normals", "out", out, torch.float32, nv * NORMAL_FLOATS, dev).view(nv, NORMAL_FLOATS)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_normals(_ptr(vertices), nv, _ptr_i32(triangles), nt, _ptr_i32(offsets), _ptr_i32(corners), _ptr(out), st),
              "mnerf_mesh_normals")
    return out


DECIMATE_REG = 1.0 / 1000  # 1 / MNERF_DECIMATE_REG_INV: the regularisation weight of mesh_decimate


def mesh_decimate_workspace_bytes(n_vertices, n_triangles, dims):
    return int(load().mnerf_mesh_decimate_workspace_bytes(int(n_vertices), int(n_triangles), int(dims[0]), int(dims[1]), int(dims[2])))


def mesh_decimate(vertices, triangles, adjacency, origin, cell, dims, vertices_out=None, triangles_out=None, vertex_map=None, counts=None,
                  workspace=None, stream=None):
    """Decimation by quadric vertex clustering (mnerf_mesh_decimate): the vertices of every cell of the grid ``origin`` (x, y, z),
    ``cell``, ``dims`` = (gx, gy, gz) become one vertex - the regularised minimiser of the cell's plane quadric, clamped to the cell -
    in ascending cell order, and the triangles that still join three cells are kept once each, in order.  ``adjacency`` = the tables
    of ``mesh_adjacency`` for this mesh.  ``vertices_out`` [capacity, 8] / ``triangles_out`` [capacity, 3] default to the input's
    sizes (upper bounds of the counts), ``vertex_map`` is an int32 [V] tensor or None (not wanted), ``counts`` a 2-element int64
    tensor.  Enqueue only: -> (vertices_out, triangles_out, counts); rows at or beyond a capacity are not written, the counts are the
    totals either way."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_decimate", vertices, triangles)
    offsets = _mesh_buffer("mesh_decimate", "offsets", adjacency[0], torch.int32, nv + 1, dev)
    corners = _mesh_buffer("mesh_decimate", "corners", adjacency[1], torch.int32, 3 * nt, dev)
    grid = _grid(origin, cell, dims)
    need = mesh_decimate_workspace_bytes(nv, nt, grid[4:])
    if need < 0 or not (np.isfinite(grid[:4]).all() and grid[3] > 0):
        raise MnerfError(f"mesh_decimate: the grid {tuple(grid[4:])} of cell {grid[3]} from {tuple(grid[:3])} is out of range")
    if vertices_out is None:
        vertices_out = torch.empty(nv, VERTEX_FLOATS, device=dev)
    if triangles_out is None:
        triangles_out = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    _mesh_args("mesh_decimate", vertices_out, triangles_out)
    if vertices_out.device != dev:
        raise MnerfError(f"mesh_decimate: vertices_out on {vertices_out.device}, the mesh on {dev}")
    if vertex_map is not None:
        vertex_map = _mesh_buffer("mesh_decimate", "vertex_map", vertex_map, torch.int32, nv, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else _mesh_buffer("mesh_decimate", "counts", counts,
                                                                                              torch.int64, 2, dev)
    workspace = export_workspace("mesh_decimate", workspace, need, dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_decimate(_ptr(vertices), _ptr_i32(triangles), nv, nt, _ptr_i32(offsets), _ptr_i32(corners), *grid,
                                      _ptr(vertices_out), vertices_out.numel() // VERTEX_FLOATS, _ptr_i32(triangles_out),
                                      triangles_out.numel() // 3, _ptr_i32(vertex_map), _ptr(counts), _ptr(workspace), st),
              "mnerf_mesh_decimate")
    return vertices_out, triangles_out, counts


# ----------------------------------------------------------------------- mesh texture (matchnerf_amd/csrc/mesh_texture.hip)

ATLAS_FLOATS = 4  # floats of one texel of an accumulation buffer (r g b | w) or an atlas (r g b a)
TEXTURE_MIN_BLOCK, TEXTURE_MAX_BLOCK, TEXTURE_MAX_POWER = 4, 64, 8


def mesh_texture_atlas(n_triangles, block):
    """The size (W, H) of the atlas of ``n_triangles`` triangles in blocks of ``block`` texels (mnerf_mesh_texture_atlas: a function
    of the two numbers only; include/mnerf.h states the layout).  Host only, needs no GPU; MnerfError beyond the header's bounds."""
    size = (C.c_int32 * 2)()
    check(load().mnerf_mesh_texture_atlas(int(n_triangles), int(block), size), "mnerf_mesh_texture_atlas")
    return int(size[0]), int(size[1])


def _texture_args(what, vertices, triangles, block, buffers):
    """the checks of ``_mesh_args`` plus the atlas: every tensor of ``buffers`` (name -> tensor) is a float32 [H, W, 4] buffer on the
    mesh's device -> (device, V, T, (W, H))"""
    import torch
    dev, nv, nt = _mesh_args(what, vertices, triangles)
    width, height = mesh_texture_atlas(nt, block)
    for name, t in buffers.items():
        _mesh_buffer(what, name, t, torch.float32, height * width * ATLAS_FLOATS, dev)
    return dev, nv, nt, (width, height)


def mesh_texture_uv(n_triangles, block, device=None, out=None, stream=None):
    """The texture coordinates of every triangle's corners (mnerf_mesh_texture_uv) -> [T, 3, 2] float32, (x / W, y / H) with the origin
    at the top-left of the atlas.  ``out``: the tensor to write into (``device`` is then its device).  Enqueue only."""
    import torch
    lib = load()
    n_triangles = int(n_triangles)
    mesh_texture_atlas(n_triangles, block)  # the bounds
    dev = out.device if out is not None else torch.device(_current_device() if device is None else device)
    if dev.type != "cuda":
        raise MnerfError(f"mesh_texture_uv: uv lies on {dev}; it is written on the GPU")
    out = _mesh_buffer("mesh_texture_uv", "uv", out, torch.float32, 6 * n_triangles, dev).view(n_triangles, 3, 2)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_texture_uv(n_triangles, int(block), _ptr(out), st), "mnerf_mesh_texture_uv")
    return out


def mesh_texture_accumulate(vertices, triangles, block, views, depth, rgb, accum, opacity=None, n_consistent=None, min_consistent=0,
                            legacy=True, min_opacity=0.5, vis_rel_tol=0.02, power=2, best=False, stream=None):
    """Add up to MNERF_MAX_VIEWS views to the accumulation buffer of a mesh's atlas (mnerf_mesh_texture_accumulate; the visibility
    test and the weights are stated in include/mnerf.h).  ``vertices`` [V, 8] / ``triangles`` [T, 3] as for ``mesh_normals``;
    ``views``, ``depth`` [K, h, w], ``opacity``, ``n_consistent``, ``rgb`` [K, h*w, 3] as for ``tsdf_integrate``; ``accum`` [H, W, 4]
    float32 of ``mesh_texture_atlas(T, block)``, the caller's, zeroed before the first call; calls accumulate.  ``power`` 0..8: the
    weight of a view is cos^power of its angle to the normal; ``best``: keep the view of the largest weight instead of the weighted
    sum.  Enqueue only: -> accum."""
    import torch
    lib = load()
    dev, nv, nt, _ = _texture_args("mesh_texture_accumulate", vertices, triangles, block, dict(accum=accum))
    _f32c(depth, "depth"), _f32c(rgb, "rgb")
    if depth.dim() != 3 or depth.shape[0] != len(views) or depth.device != dev:
        raise MnerfError(f"mesh_texture_accumulate: depth {tuple(depth.shape)} on {depth.device} is not [{len(views)}, h, w] on {dev}")
    k, h, w = (int(x) for x in depth.shape)
    if rgb.numel() != 3 * depth.numel() or rgb.device != dev:
        raise MnerfError(f"mesh_texture_accumulate: rgb {tuple(rgb.shape)} on {rgb.device} is not [{k}, {h * w}, 3] on {dev}")
    if opacity is not None and (_f32c(opacity, "opacity").shape != depth.shape or opacity.device != dev):
        raise MnerfError(f"mesh_texture_accumulate: opacity {tuple(opacity.shape)} on {opacity.device} does not match depth "
                         f"{tuple(depth.shape)}")
    if n_consistent is not None and (n_consistent.dtype != torch.int32 or n_consistent.numel() != depth.numel()
                                     or not n_consistent.is_contiguous() or n_consistent.device != dev):
        raise MnerfError(f"mesh_texture_accumulate: n_consistent must be a contiguous int32 tensor of {depth.numel()} elements on {dev}")
    if int(power) != power or not 0 <= int(power) <= TEXTURE_MAX_POWER:
        raise MnerfError(f"mesh_texture_accumulate: power={power!r} is no integer in 0..{TEXTURE_MAX_POWER}")
    arr = views if isinstance(views, C.Array) else view_array(views)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_texture_accumulate(_ptr(vertices), _ptr_i32(triangles), nv, nt, int(block), arr, k, h, w, int(bool(legacy)),
                                                _ptr(depth), _ptr(opacity), _ptr_i32(n_consistent), int(min_consistent), _ptr(rgb),
                                                float(min_opacity), float(vis_rel_tol), int(power), int(bool(best)), _ptr(accum), st),
              "mnerf_mesh_texture_accumulate")
    return accum


def mesh_texture_resolve(vertices, triangles, block, accum, best=False, out=None, stream=None):
    """The atlas of an accumulation buffer (mnerf_mesh_texture_resolve) -> [H, W, 4] float32 ``r g b a``: the weighted mean (``best``:
    the stored colour) with a = 1 where a view saw the surface, the blend of the triangle's vertex colours with a = 0 where none did,
    zeros where no triangle owns the texel.  ``out`` may be ``accum`` (in place); default a new tensor.  Enqueue only."""
    import torch
    lib = load()
    buffers = dict(accum=accum) if out is None else dict(accum=accum, atlas=out)
    dev, nv, nt, (width, height) = _texture_args("mesh_texture_resolve", vertices, triangles, block, buffers)
    if out is None:
        out = torch.zeros(height, width, ATLAS_FLOATS, device=dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_texture_resolve(_ptr(vertices), _ptr_i32(triangles), nv, nt, int(block), int(bool(best)), _ptr(accum),
                                             _ptr(out), st), "mnerf_mesh_texture_resolve")
    return out.view(height, width, ATLAS_FLOATS)


# ----------------------------------------------------------------------- mesh raster (matchnerf_amd/csrc/mesh_raster.hip)

RGBA_FLOATS = 4  # floats of one pixel of a shaded frame (r g b a) or of a normal frame (nx ny nz 0)


def mesh_raster_workspace_bytes(height, width):
    """The bytes of the key buffer of a ``height`` x ``width`` frame (mnerf_mesh_raster_workspace_bytes: 8 per pixel); -1 for a frame
    the rasterizer does not take.  Host only."""
    return int(load().mnerf_mesh_raster_workspace_bytes(int(height), int(width)))


def _frame(what, hw):
    h, w = int(hw[0]), int(hw[1])
    if mesh_raster_workspace_bytes(h, w) < 0:
        raise MnerfError(f"{what}: a frame of {h}x{w} is out of range")
    return h, w


def mesh_raster(vertices, triangles, view, hw, legacy=True, out=None, workspace=None, stream=None):
    """The mesh seen from one camera (mnerf_mesh_raster; include/mnerf.h "MESH RASTER" states the coverage rule) -> (face int32
    [h, w]: the triangle every pixel sees, -1 where none; depth float32 [h, w]: its camera-z, 0 where none; bary float32 [h, w, 2]:
    the perspective-correct weights of the triangle's vertices 1 and 2).  ``vertices`` [V, 8] / ``triangles`` [T, 3] as for
    ``mesh_normals``; ``view``: one ``View`` - extr, the intr of the (h, w) grid, near_ / far_ = the depths that may win a pixel.
    ``out``: the three tensors to write into; ``workspace``: ``mesh_raster_workspace_bytes(h, w)`` bytes, reused across views.
    Enqueue only; the same bytes on every run."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_raster", vertices, triangles)
    h, w = _frame("mesh_raster", hw)
    out = (None, None, None) if out is None else out
    face = _mesh_buffer("mesh_raster", "face", out[0], torch.int32, h * w, dev).view(h, w)
    depth = _mesh_buffer("mesh_raster", "depth", out[1], torch.float32, h * w, dev).view(h, w)
    bary = _mesh_buffer("mesh_raster", "bary", out[2], torch.float32, 2 * h * w, dev).view(h, w, 2)
    workspace = export_workspace("mesh_raster", workspace, mesh_raster_workspace_bytes(h, w), dev)
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_raster(_ptr(vertices), _ptr_i32(triangles), nv, nt, C.byref(view), h, w, int(bool(legacy)), _ptr_i32(face),
                                    _ptr(depth), _ptr(bary), _ptr(workspace), workspace.numel() * workspace.element_size(), st),
              "mnerf_mesh_raster")
    return face, depth, bary


def mesh_shade(vertices, triangles, face, bary, view, atlas=None, block=0, normals=False, out=None, stream=None):
    """Shade a rastered frame (mnerf_mesh_shade) -> rgba float32 [h, w, 4], or (rgba, normal [h, w, 4]) with ``normals``: the blend of
    the hit triangle's vertex colours, or - with ``atlas`` [H, W, 4] of ``mesh_texture_atlas(T, block)`` - the bilinear value of the
    atlas at the hit point; a = 1 on a hit and 0 0 0 0 elsewhere; the normal is the face's, unit length, turned towards the camera.
    ``face`` [h, w] / ``bary`` [h, w, 2] as ``mesh_raster`` wrote them for ``view``.  ``out``: rgba, or the pair, to write into.
    Enqueue only."""
    import torch
    lib = load()
    dev, nv, nt = _mesh_args("mesh_shade", vertices, triangles)
    if face.dim() != 2:
        raise MnerfError(f"mesh_shade: face {tuple(face.shape)} is no [h, w] frame")
    h, w = _frame("mesh_shade", face.shape)
    face = _mesh_buffer("mesh_shade", "face", face, torch.int32, h * w, dev)
    bary = _mesh_buffer("mesh_shade", "bary", bary, torch.float32, 2 * h * w, dev)
    width = height = 0
    if atlas is not None:
        width, height = mesh_texture_atlas(nt, block)
        atlas = _mesh_buffer("mesh_shade", "atlas", atlas, torch.float32, height * width * ATLAS_FLOATS, dev)
    out = out if isinstance(out, (tuple, list)) else (out, None)
    rgba = _mesh_buffer("mesh_shade", "rgba", out[0], torch.float32, h * w * RGBA_FLOATS, dev).view(h, w, RGBA_FLOATS)
    normal = _mesh_buffer("mesh_shade", "normal", out[1], torch.float32, h * w * RGBA_FLOATS, dev).view(h, w, RGBA_FLOATS) if normals else None
    with _on(dev, stream) as st:
        check(lib.mnerf_mesh_shade(_ptr(vertices), _ptr_i32(triangles), nv, nt, _ptr_i32(face), _ptr(bary), h, w, _ptr(atlas), height, width,
                                   int(block), C.byref(view), _ptr(rgba), _ptr(normal), st), "mnerf_mesh_shade")
    return (rgba, normal) if normals else rgba
