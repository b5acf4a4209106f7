"""ctypes binding of libishap_hip.so (the C ABI declared in include/ishap.h).

The product path has no CPU fallback: if the library is missing or a call fails,
this module raises.  Build with `python -m ishapediting_amd.build`.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libishap_hip.so")

c_float_p = C.POINTER(C.c_float)
c_void_p = C.c_void_p


class UNetConfigC(C.Structure):
    _fields_ = [("image_size", C.c_int), ("in_channels", C.c_int), ("model_channels", C.c_int),
                ("out_channels", C.c_int), ("num_res_blocks", C.c_int), ("n_mult", C.c_int),
                ("channel_mult", C.c_int * 8), ("n_att", C.c_int), ("attention_ds", C.c_int * 8),
                ("num_head_channels", C.c_int), ("max_batch", C.c_int)]


class StepCoefs(C.Structure):
    _fields_ = [("min_log", C.c_float), ("max_log", C.c_float), ("sqrt_recip", C.c_float),
                ("sqrt_recipm1", C.c_float), ("coef1", C.c_float), ("coef2", C.c_float),
                ("nonzero", C.c_float), ("clip_denoised", C.c_int), ("mode", C.c_int),
                ("ddim_a", C.c_float), ("ddim_b", C.c_float), ("ddim_sigma", C.c_float),
                ("rng", C.c_int), ("rng_seed", C.c_ulonglong), ("rng_offset", C.c_ulonglong), ("noise_out", c_void_p)]


class DragBatchArgsC(C.Structure):
    _fields_ = [("E", C.c_int), ("W", C.c_int), ("ld", C.c_int), ("Cc", C.c_int), ("chmap", c_void_p), ("sources", c_void_p),
                ("targets", c_void_p), ("handle_offsets", C.POINTER(C.c_int)), ("r", C.c_int), ("voxel", C.c_float),
                ("cof", C.POINTER(C.c_float)), ("l1", C.c_int), ("orig_stride", C.c_longlong), ("scratch", c_void_p),
                ("scratch_bytes", C.c_longlong), ("weights", c_void_p), ("weights_stride", C.c_longlong)]     # the last two: ABI 17


class RegionPrimC(C.Structure):
    _fields_ = [("kind", C.c_int), ("role", C.c_int), ("a", C.c_double * 3), ("b", C.c_double * 3)]


class IgemmBufC(C.Structure):
    _fields_ = [("ptr", c_void_p), ("bytes", C.c_longlong)]


class IgemmDescC(C.Structure):
    _fields_ = ([(f, C.c_int) for f in ("M", "N", "Cin", "taps", "K2", "H", "W", "ldx", "ldx2", "ldw", "ldo", "ldr", "ups",
                                        "res_ups", "out_mode", "pending", "chunk_tiles")] +
                [(f, IgemmBufC) for f in ("X", "X2", "Wt", "out", "bias", "bias2", "res", "ws", "stat_out", "gb_x", "gb_stats",
                                          "gb_gamma", "gb_beta", "gb_emb", "gb_csums")] +
                [("gb_emb_ld", C.c_int), ("gb_film", C.c_int), ("gb_act", C.c_int)])


class AttnDescC(C.Structure):
    _fields_ = ([(f, C.c_int) for f in ("pass_", "N", "T", "C", "heads", "d", "xcd_map")] +
                [(f, IgemmBufC) for f in ("qkv", "out", "lse", "dout", "dqkv")])


class Attn8DescC(C.Structure):
    _fields_ = ([(f, C.c_int) for f in ("N", "C", "heads")] +
                [(f, IgemmBufC) for f in ("xn", "wqkv", "bqkv", "wproj", "qkv", "aout", "lse", "slices", "flags")])


class GroupNormDescC(C.Structure):
    _fields_ = ([(f, C.c_int) for f in ("backward", "N", "H", "W", "C", "route", "film", "act", "pool", "split", "gmode",
                                        "sums_ready", "csplit", "emb_ld")] +
                [(f, c_void_p) for f in ("gamma", "beta", "emb", "scratch", "x", "x2", "xcopy", "out", "xpool", "stats_out", "sums",
                                         "sums2", "g", "stats", "add", "add2", "dx", "dx2", "csums", "ws")] +
                [(f, C.c_int) for f in ("nslab", "ldr", "res_ups", "reserved_")] + [("zstride", C.c_longlong)] +
                [(f, c_void_p) for f in ("bias", "bias2", "res", "ya")])


class DecoderWeightsC(C.Structure):
    _fields_ = [("B", c_void_p), ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
                ("w3", c_void_p), ("b3", c_void_p)]


class CameraC(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("centre", C.c_float * 3), ("up", C.c_float * 3), ("fov_y_deg", C.c_float),
                ("near", C.c_float), ("far", C.c_float)]


# every symbol include/ishap.h declares: (restype, argtypes)
SYMBOLS = {
    "ishap_last_error": (C.c_char_p, []),
    "ishap_version": (C.c_int, []),
    "ishap_device_status": (C.c_int, []),
    "ishap_rendezvous_would_grant": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ishap_group_norm32_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "ishap_group_norm32": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_group_norm32_backward": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_group_norm32_plan": (C.c_int, [C.c_int] * 11 + [C.POINTER(C.c_int)] * 8 + [C.c_char_p, C.c_int]),
    "ishap_group_norm32_run": (C.c_int, [C.POINTER(GroupNormDescC), C.c_int, c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.c_char_p, C.c_int]),
    "ishap_unet_create": (C.c_int, [C.POINTER(UNetConfigC), C.c_int, C.POINTER(c_void_p)]),
    "ishap_unet_destroy": (None, [c_void_p]),
    "ishap_unet_num_params": (C.c_int, [c_void_p]),
    "ishap_unet_param_info": (C.c_int, [c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_longlong)]),
    "ishap_unet_load_param": (C.c_int, [c_void_p, C.c_char_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_unet_params_loaded": (C.c_int, [c_void_p]),
    "ishap_unet_forward": (C.c_int, [c_void_p, c_void_p, c_float_p, C.c_int, C.c_int, c_void_p, c_void_p, C.c_int,
                                     c_void_p]),
    "ishap_unet_tap_shape": (C.c_int, [c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ishap_unet_tap_ptr": (c_void_p, [c_void_p]),
    "ishap_unet_copy_tap": (C.c_int, [c_void_p, c_void_p, c_void_p]),
    "ishap_unet_block_output": (C.c_int, [c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), c_void_p,
                                          c_void_p]),
    "ishap_unet_block_grad": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), c_void_p,
                                        c_void_p]),
    "ishap_unet_workspace_bytes": (C.c_longlong, [c_void_p]),
    "ishap_unet_join_tail": (C.c_int, [c_void_p, c_void_p]),
    "ishap_unet_run_tail": (C.c_int, [c_void_p]),
    "ishap_unet_snapshot_save": (C.c_int, [c_void_p, c_void_p]),
    "ishap_unet_snapshot_restore": (C.c_int, [c_void_p, c_void_p]),
    "ishap_unet_snapshot_drop": (C.c_int, [c_void_p]),
    "ishap_unet_snapshot_bytes": (C.c_longlong, [c_void_p]),
    "ishap_unet_marks": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_int, c_void_p, c_void_p]),
    "ishap_unet_prepare_timesteps": (C.c_int, [c_void_p, c_void_p, C.c_int, c_void_p]),
    "ishap_unet_backward_input": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_unet_backward_from_output": (C.c_int, [c_void_p, c_void_p, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_triplane_points_loss_grad": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, c_void_p, c_void_p,
                                                  c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_x0_grad_to_cotangent": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                             c_void_p, c_void_p, c_void_p]),
    "ishap_ddpm_step": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.POINTER(StepCoefs), C.c_int, C.c_int,
                                  C.c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_ddpm_step_guided": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.POINTER(StepCoefs), C.c_int, C.c_int, C.c_int,
                                         c_void_p, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_ddpm_step_guided_scales": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.POINTER(StepCoefs), C.c_int, C.c_int,
                                                C.c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_guided_update": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_float, c_void_p, C.c_longlong, c_void_p,
                                      c_void_p]),
    "ishap_axpby": (C.c_int, [c_void_p, c_void_p, C.c_float, C.c_float, C.c_longlong, c_void_p, c_void_p]),
    "ishap_drag_batch_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    "ishap_drag_batch_setup": (C.c_int, [C.POINTER(DragBatchArgsC), c_void_p]),
    "ishap_drag_batch_loss_grad": (C.c_int, [C.POINTER(DragBatchArgsC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_drag_batch_loss_cotangent": (C.c_int, [C.POINTER(DragBatchArgsC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p]),
    "ishap_drag_track_scratch_bytes": (C.c_longlong, [C.c_int] * 5),
    "ishap_drag_track": (C.c_int, [c_void_p, c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p,
                                   C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_drag_batch_retarget": (C.c_int, [C.POINTER(DragBatchArgsC), c_void_p, c_void_p, C.c_float, C.c_float, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    "ishap_drag_batch_retarget_each": (C.c_int, [C.POINTER(DragBatchArgsC), c_void_p, c_void_p, C.POINTER(C.c_float),
                                                 C.POINTER(C.c_float), c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_region_plane_weights_scratch_bytes": (C.c_longlong, [C.c_int]),
    "ishap_region_plane_weights": (C.c_int, [c_void_p, C.c_int, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                             c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_region_plane_marks": (C.c_int, [c_void_p, C.c_int, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p,
                                           c_void_p, C.c_longlong, c_void_p]),
    "ishap_region_plane_feather_scratch_bytes": (C.c_longlong, [C.c_int]),
    "ishap_region_plane_feather": (C.c_int, [c_void_p, C.c_int, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                             c_void_p, C.c_int, c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_edt_scratch_bytes": (C.c_longlong, [C.c_int] * 4),
    "ishap_edt": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_region_select": (C.c_int, [c_void_p, C.c_int, C.c_float, c_void_p, C.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_region_handles_scratch_bytes": (C.c_longlong, [C.c_int, C.c_int]),
    "ishap_region_handles": (C.c_int, [c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), c_void_p, c_void_p, c_void_p, c_void_p,
                                       C.c_longlong, c_void_p]),
    "ishap_region_transform": (C.c_int, [c_void_p, C.c_int, C.POINTER(C.c_double), c_void_p, c_void_p, c_void_p]),
    "ishap_grad_to_scaled_f16": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_planes_prepare": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_int, c_void_p, c_void_p]),
    "ishap_triplane_fit_loss_grad": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, c_void_p, c_void_p,
                                               C.c_longlong, c_void_p, c_void_p, C.c_longlong, C.c_float, c_void_p, c_void_p,
                                               c_void_p]),
    "ishap_triplane_reg_adam_step": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int, c_void_p, C.c_double,
                                               C.c_double, C.c_double, C.c_double, C.c_float, C.c_float, c_void_p, c_void_p,
                                               c_void_p]),
    "ishap_triplane_reg_values": (C.c_int, [c_void_p, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_triplane_decode_points": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, C.c_longlong,
                                               c_void_p, c_void_p]),
    "ishap_triplane_field_grad": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, C.c_longlong, c_void_p,
                                            c_void_p, c_void_p]),
    "ishap_constraint_setup_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_int]),
    "ishap_constraint_setup": (C.c_int, [c_void_p, C.c_longlong, C.c_int, c_void_p, c_void_p, c_void_p, c_void_p, C.c_longlong,
                                         c_void_p]),
    "ishap_constraint_loss_grad": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, c_void_p, c_void_p,
                                             C.c_longlong, C.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    "ishap_triplane_project": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, C.c_longlong, C.c_int,
                                         C.c_float, C.c_float, C.c_float, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "ishap_surface_scratch_bytes": (C.c_longlong, [C.c_int]),
    "ishap_surface_count": (C.c_int, [c_void_p, C.c_int, C.c_float, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_surface_emit": (C.c_int, [c_void_p, C.c_int, C.c_float, C.c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ishap_mesh_smooth_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong]),
    "ishap_mesh_smooth": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, C.c_int, C.c_float, c_void_p, C.c_longlong, c_void_p]),
    "ishap_chamfer": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p]),
    "ishap_mesh_tri_areas": (C.c_int, [c_void_p, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_mesh_points_on_tris": (C.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_mesh_occupancy": (C.c_int, [c_void_p, c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_mesh_distance_scratch_bytes": (C.c_longlong, [C.c_longlong]),
    "ishap_mesh_distance": (C.c_int, [c_void_p, c_void_p, C.c_longlong, c_void_p, C.c_longlong, C.c_int, c_void_p, c_void_p,
                                      c_void_p, C.c_longlong, c_void_p]),
    "ishap_mesh_distance_scratch_bytes_sdf": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int]),
    "ishap_hausdorff": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p]),
    "ishap_winding_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong]),
    "ishap_mesh_winding": (C.c_int, [c_void_p, c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p, C.c_longlong,
                                     c_void_p]),
    "ishap_cloud_winding": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p,
                                      C.c_longlong, c_void_p]),
    "ishap_cloud_areas": (C.c_int, [c_void_p, C.c_longlong, C.c_int, c_void_p, c_void_p]),
    "ishap_cloud_knn": (C.c_int, [c_void_p, C.c_longlong, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_cloud_normals": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_cloud_orient_scratch_bytes": (C.c_longlong, [C.c_longlong]),
    "ishap_cloud_orient": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_longlong, C.c_int, c_void_p, C.c_longlong,
                                     C.POINTER(C.c_int), c_void_p]),
    "ishap_volume_label": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, c_void_p, c_void_p]),
    "ishap_volume_components_scratch_bytes": (C.c_longlong, [C.c_longlong]),
    "ishap_volume_components_count": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_volume_components_emit": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p, c_void_p]),
    "ishap_volume_flip": (C.c_int, [c_void_p, c_void_p, c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, c_void_p, C.c_longlong,
                                    c_void_p, c_void_p]),
    "ishap_group_field_stats": (C.c_int, [c_void_p, c_void_p, C.c_int, C.c_longlong, C.c_int, c_void_p, c_void_p]),
    "ishap_arap_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_longlong]),
    "ishap_arap": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p, C.c_longlong, C.c_int, C.c_double,
                             C.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, C.c_longlong, c_void_p]),
    "ishap_nearest_vertices": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_render_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong, C.c_int, C.c_int]),
    "ishap_render_mesh": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p, C.c_int,
                                    C.POINTER(CameraC), C.c_int, C.c_int, c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "ishap_unproject": (C.c_int, [C.POINTER(CameraC), C.c_int, C.c_int, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_profile_begin": (C.c_int, []),
    "ishap_profile_end": (C.c_int, [C.POINTER(C.c_double), C.c_int]),
    "ishap_profile_shapes": (C.c_int, [C.c_char_p, C.c_int]),
    "ishap_igemm_plan": (C.c_int, [C.c_int] * 10 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "ishap_igemm_run": (C.c_int, [C.POINTER(IgemmDescC), C.c_int, c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "ishap_igemm_reduce": (C.c_int, [C.POINTER(IgemmDescC), C.c_int, C.c_int, c_void_p]),
    "ishap_attention_run": (C.c_int, [C.POINTER(AttnDescC), C.c_int, c_void_p, C.c_char_p, C.c_int]),
    "ishap_attention8_run": (C.c_int, [C.POINTER(Attn8DescC), C.c_int, C.c_int, c_void_p, C.POINTER(C.c_int)]),
    "ishap_triplane_decode_grid": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, C.c_int,
                                             c_void_p, c_void_p]),
    "ishap_sparse_bricks_per_axis": (C.c_int, [C.c_int]),
    "ishap_sparse_seed_range": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ishap_sparse_seed_volume": (C.c_int, [c_void_p, C.c_int, C.c_float, C.c_int, c_void_p, c_void_p]),
    "ishap_sparse_compact_scratch_bytes": (C.c_longlong, [C.c_int]),
    "ishap_sparse_compact": (C.c_int, [c_void_p, C.c_int, C.c_int, C.c_int, c_void_p, c_void_p, C.c_longlong, c_void_p, c_void_p,
                                       C.c_longlong, c_void_p]),
    "ishap_triplane_decode_bricks": (C.c_int, [c_void_p, C.c_int, C.POINTER(DecoderWeightsC), c_void_p, C.c_int, c_void_p,
                                               C.c_longlong, c_void_p, c_void_p]),
    "ishap_sparse_reach_bytes": (C.c_longlong, [C.c_longlong]),
    "ishap_sparse_grow": (C.c_int, [c_void_p, c_void_p, C.c_longlong, C.c_int, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "ishap_sparse_surface_scratch_bytes": (C.c_longlong, [C.c_int, C.c_longlong]),
    "ishap_sparse_surface_count": (C.c_int, [c_void_p, c_void_p, C.c_longlong, C.c_int, C.c_float, c_void_p, c_void_p, c_void_p,
                                             C.c_longlong, c_void_p, c_void_p]),
    "ishap_sparse_surface_emit": (C.c_int, [c_void_p, c_void_p, C.c_longlong, C.c_int, C.c_float, c_void_p, c_void_p, c_void_p,
                                            C.c_longlong, c_void_p, c_void_p, c_void_p]),
    "ishap_mesh_simplify_scratch_bytes": (C.c_longlong, [C.c_longlong, C.c_longlong, C.POINTER(C.c_int)]),
    "ishap_mesh_simplify_count": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_double,
                                            C.POINTER(C.c_int), C.c_int, c_void_p, C.c_longlong, c_void_p, c_void_p]),
    "ishap_mesh_simplify_emit": (C.c_int, [c_void_p, C.c_longlong, c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_double,
                                           C.POINTER(C.c_int), C.c_int, C.c_double, c_void_p, C.c_longlong, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
}

ABI = 27          # the ishap_version() this module's SYMBOLS and structures describe

_lib = None


def lib():
    """Load (once) and return the shared library; raise if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is required (no CPU fallback exists). "
                "Build it with `python -m ishapediting_amd.build`.")
        # One HIP runtime per process: torch ships its own libamdhip64 and must be the one that is resident
        # (torch owns the device memory and streams we are handed), so load it before our library resolves
        # its libamdhip64.so.N dependency by SONAME.
        import torch  # noqa: F401
        tlib = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tlib):
            C.CDLL(tlib, mode=C.RTLD_GLOBAL)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)     # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        # which ABI added which symbol: the version notes of include/ishap.h
        if l.ishap_version() < ABI:
            raise RuntimeError(f"{LIB_PATH} is an older build (ABI {l.ishap_version()} < {ABI}): rebuild with `python -m ishapediting_amd.build`")
        _lib = l
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().ishap_last_error()
        raise RuntimeError(f"libishap_hip: {msg.decode() if msg else 'error'} (code {rc})")


def ptr(t):
    """Device (or host) address of a torch tensor; None -> NULL."""
    return None if t is None else t.data_ptr()


def stream_ptr(device=None):
    """hipStream_t of torch's current stream, so library work is ordered with torch ops."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class ScratchError(RuntimeError):
    """a *_scratch_bytes entry refused its sizes (a negative return)"""


def need_gpu(t_or_device, what: str, verb: str = "runs"):
    """The GPU `what` runs on: the device of a tensor, a given device as it is, or torch's current GPU for None.  Raises for a
    host tensor, and for None without a GPU: there is no CPU fallback."""
    import torch
    if torch.is_tensor(t_or_device):
        if t_or_device.is_cuda:
            return t_or_device.device
    elif t_or_device is not None:
        return torch.device(t_or_device)
    elif torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    raise RuntimeError(f"{what} {verb} on the GPU (libishap_hip.so); there is no CPU fallback")


def tensor(x, dtype, device=None, shape=None):
    """`x` (a tensor, or anything numpy.asarray takes) detached, on `device` (None: where it is) as `dtype`, reshaped to
    `shape` when given, contiguous: the input's own storage when it already conforms."""
    import torch
    if not torch.is_tensor(x):
        import numpy as np
        x = torch.from_numpy(np.asarray(x))
    t = x.detach().to(device=device, dtype=dtype)
    return (t if shape is None else t.reshape(shape)).contiguous()


def scratch(device, name: str, *sizes):
    """(uint8 tensor on `device`, its bytes) of the size the `name` (*_scratch_bytes) entry states for `sizes`"""
    import torch
    nbytes = int(getattr(lib(), name)(*sizes))
    if nbytes < 0:
        raise ScratchError(f"{name}{sizes}: the library refuses these sizes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def call(device, name: str, *args, stream=True):
    """Run the library entry `name` with `device` current and raise on a non-zero return code.  The last argument is the
    stream: torch's current one on `device` (stream=True), one fetched before (a stream_ptr value), or none (stream=False,
    for entries that take no stream)."""
    import torch
    with torch.cuda.device(device):
        if stream is True:
            args += (stream_ptr(device),)
        elif stream is not False:
            args += (stream,)
        check(getattr(lib(), name)(*args))
