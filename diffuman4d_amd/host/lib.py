"""ctypes binding of libdm4d.so (C ABI declared in include/dm4d.h).

The library is the product's only compute path: there is no CPU or PyTorch fallback.  Loading
fails loudly if the shared object has not been built (``python -m diffuman4d_amd.build``).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_LIB_PATH = Path(__file__).resolve().parent.parent / "libdm4d.so"
_lib = None

_vp, _i, _i64, _f, _u = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint

# name -> (restype, argtypes); mirrors include/dm4d.h exactly (tests/test_abi.py checks the header)
SIGNATURES = {
    "dm4d_version": (_i, []),
    "dm4d_last_error": (C.c_char_p, []),
    "dm4d_gemm_bf16": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp, _i64, _i, _vp,
                            _i64, _u, _f]),
    "dm4d_conv3x3_nhwc_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp,
                                    _i64, _f]),
    "dm4d_conv3x3_nhwc_bf16_ws": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp,
                                    _i64, _f, _vp, C.c_size_t]),
    "dm4d_conv3x3_nhwc_bf16_flags": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp,
                                          _i64, _f, _u]),
    "dm4d_conv3x3_ws_bytes": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "dm4d_conv2d_direct_nhwc_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "dm4d_conv2d_direct_nhwc_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "dm4d_groupnorm_ws_bytes": (C.c_size_t, [_i, _i, _i]),
    "dm4d_groupnorm_nhwc_bf16": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "dm4d_layernorm_bf16": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _f]),
    "dm4d_attention_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _f]),
    "dm4d_attention_kv_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _f]),
    "dm4d_attention_qscaled_kv_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i]),
    "dm4d_softmax_rows_bf16": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _f]),
    "dm4d_softmax_rows_f32in_bf16": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _f]),
    "dm4d_timestep_embedding_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_silu_bf16": (_i, [_vp, _vp, _vp, _i64]),
    "dm4d_pack_model_input_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_cfg_ddim_step_bf16": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f, _i]),
    "dm4d_cfg_linear_step_bf16": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_cfg_multistep_step_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_vae_sample_bf16": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i, _f]),
    "dm4d_scale_pad_bf16": (_i, [_vp, _vp, _i64, _vp, _i, _i64, _i, _f]),
    "dm4d_resize_nchw_f32_to_nhwc_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "dm4d_plucker_latent_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_postprocess_images_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_resize_aa_nchw_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i]),
    "dm4d_conv_up2x_prepare_bf16": (_i, [_vp, _vp, _vp, _i, _i]),
    "dm4d_conv_up2x_nhwc_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "dm4d_ff_geglu_prepare_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i]),
    "dm4d_ff_geglu_supported": (_i, [_i, _i]),
    "dm4d_ff_geglu_fused_bf16": (_i, [_vp, _vp, _i64, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i, _i, _i]),
    "dm4d_attn_out_ff_geglu_fused_bf16": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i,
                                                _i]),
    "dm4d_l0_linear_fused_supported": (_i, [_i]),
    "dm4d_proj_in_ln_qkv_fused_bf16": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i]),
    # parity precision (fp32 tensors between kernels, two-term bf16 operands)
    "dm4d_split_f32": (_i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i, _vp, _i64, _i64, _i, _i, _f, _i]),
    "dm4d_groupnorm_f32_ws_bytes": (C.c_size_t, [_i, _i, _i]),
    "dm4d_groupnorm_nhwc_f32_split": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "dm4d_layernorm_f32_split": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _f]),
    "dm4d_softmax_rows_f32_split": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _f]),
    "dm4d_attention_split_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _f]),
    "dm4d_timestep_embedding_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_pack_model_input_f32_split": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_cfg_ddim_step_f32": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f, _i]),
    "dm4d_cfg_linear_step_f32": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_cfg_multistep_step_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i, _i, _i, _f]),
    "dm4d_vae_sample_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i, _f]),
    "dm4d_resize_nchw_f32_to_nhwc_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "dm4d_plucker_latent_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_postprocess_images_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_nhwc_to_nchw_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    # fp16 precision (fp32 tensors between kernels, single-term fp16 MFMA operands)
    "dm4d_gemm_f16": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp, _i64, _i, _vp, _i64, _u, _f, _i, _f]),
    "dm4d_conv3x3_nhwc_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _f, _u, _vp,
                                   C.c_size_t]),
    "dm4d_conv_up2x_prepare_f16": (_i, [_vp, _vp, _vp, _i, _i]),
    "dm4d_conv_up2x_nhwc_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _u]),
    "dm4d_to_f16_f32": (_i, [_vp, _vp, _i64, _i64, _i, _vp, _i64, _i, _vp, _i64, _i64, _i, _i, _f]),
    "dm4d_groupnorm_nhwc_f32_f16": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "dm4d_groupnorm_nhwc_f16_f16": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "dm4d_groupnorm_nhwc_f32_f16_raw": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _vp]),
    "dm4d_layernorm_f32_f16": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _f]),
    "dm4d_groupnorm_f32_f16_general": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp]),
    "dm4d_layernorm_f32_f16_general": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _f]),
    "dm4d_softmax_rows_f32_f16": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _f]),
    "dm4d_attention_qscaled_kv_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i]),
    "dm4d_attention_hd_qscaled_kv_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i]),
    "dm4d_attention_hd_qscaled_kv_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _i]),
    "dm4d_attention_hd_split_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _i, _i, _f,
                                          _i]),
    "dm4d_attn_out_ff_geglu_fused_f16": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i,
                                               _i]),
    "dm4d_pack_model_input_f32_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    # the per-sweep prefix cache (host/pipeline.py): model input of a subset of a window's frames, and the row mover
    "dm4d_pack_model_input_rows_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_pack_model_input_rows_f32_split": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_pack_model_input_rows_f32_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_rows_move": (_i, [_vp, _vp, _i]),
    "dm4d_groupnorm_plan_batch": (_i, [_i]),
    "dm4d_tune_set_gemm_config": (_i, [_i]),
    "dm4d_tune_set_groupnorm_resident": (_i, [_i]),
    "dm4d_nchw_to_nhwc_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_nhwc_to_nchw_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    # captured frames: crop + Pillow-exact bicubic resize + the dataset's fp32 epilogue (host/capture.py)
    "dm4d_capture_crop_resize_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i, _i]),
    # the same resize into uint8 cells kept on the device, and cells -> samples (host/capture_cache.py, device_cache=True)
    "dm4d_capture_crop_resize_packed_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i, _i]),
    "dm4d_capture_unpack_cells_f32": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i]),
    # box + byte sum of planes decoded on the device, and rectangle masks (host/capture.py, device_decode=True)
    "dm4d_capture_plane_stats_ws_bytes": (C.c_size_t, [_i, _i64]),
    "dm4d_capture_plane_stats_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64]),
    "dm4d_capture_fill_rects_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i]),
    # result evaluation: composite + nearest resize + mask crop + PSNR / SSIM of a batch of image pairs (host/metrics.py)
    "dm4d_eval_ws_bytes": (C.c_size_t, [_i, _i, _i]),
    "dm4d_eval_psnr_ssim_f64": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _i, _i]),
    # LPIPS-VGG: the steps around the VGG-16 convolutions (host/lpips.py)
    "dm4d_lpips_input_split": (_i, [_vp, _vp, _vp, _i64, _i64, _i, _i, _vp]),
    "dm4d_lpips_relu_pool_split": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "dm4d_lpips_ws_bytes": (C.c_size_t, [_i, _i]),
    "dm4d_lpips_tap_distance_f64": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp]),
    # visual-hull carving: masks to bits, then flags + scan + gather per chunk of the voxel grid (host/vhull.py)
    "dm4d_vhull_pack_masks": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "dm4d_vhull_pack_masks_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_vhull_ws_bytes": (C.c_size_t, [_i64]),
    "dm4d_vhull_carve_chunk": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i, _i, _i, _i, _i64, _i64, _vp, _i64, _vp, _vp, _i64]),
    # skeleton triangulation: one wave per (frame, keypoint), and the projection of the points into cameras (host/triang.py)
    "dm4d_triangulate_points_f64": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "dm4d_project_points_f64": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    # skeleton maps: a batch of frames' draw calls rasterised per output tile in LDS + Pillow's bicubic resize (host/skeleton.py)
    "dm4d_skeleton_draw_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    # skeleton maps from poses_3d: project + plan on the device, and the draw of a device plan (host/skeleton.py draw_skeleton_maps_kp3d)
    "dm4d_skeleton_plan_kp3d": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _f, _f,
                                     _vp, _vp, _vp]),
    "dm4d_skeleton_draw_planned_u8": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    # bounding box + box mask of drawn maps, for the dataset's skeleton-only targets (host/capture.py, skeleton_source="kp2d")
    "dm4d_skeleton_box_mask_ws_bytes": (C.c_size_t, [_i, _i, _i]),
    "dm4d_skeleton_box_mask_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64]),
    # result images: crop restore onto a white canvas and the baseline JPEG scan of a batch of images (host/jpeg.py)
    "dm4d_restore_crop_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i64]),
    "dm4d_jpeg_scan_bound": (C.c_size_t, [_i, _i]),
    "dm4d_jpeg_ws_bytes": (C.c_size_t, [_i64, _i]),
    "dm4d_jpeg_encode_rgb_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    # keypoint prediction around a caller-named pose network: composite + warp + normalise, mask box, UDP/DARK decode (host/pose.py)
    "dm4d_pose_input_u8_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i, _i]),
    "dm4d_pose_mask_box_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp]),
    "dm4d_pose_udp_decode_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    # person boxes around a caller-named detector: composite + keep-ratio resize + pad + normalise, and threshold + top-k + NMS
    # (host/detect.py)
    "dm4d_detect_input_u8_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i]),
    "dm4d_detect_select_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp]),
    # foreground masks around a caller-named matting network: rotate + bilinear resize + normalise, and logits -> bytes + bicubic
    # resize + rotate back (host/matting.py)
    "dm4d_matting_input_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i, _i, _i, _i]),
    "dm4d_matting_mask_f16_u8": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i, _i, _i]),
    # complete PNG files (L and RGBA) of a batch of images, deflate and checksums included (host/png.py)
    "dm4d_png_bound": (C.c_size_t, [_i, _i, _i]),
    "dm4d_png_ws_bytes": (C.c_size_t, [_i64, _i64, _i]),
    "dm4d_png_encode_u8": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp]),
    # complete lossless WebP files of a batch of RGB images (host/webp.py)
    "dm4d_webp_bound": (C.c_size_t, [_i, _i]),
    "dm4d_webp_ws_bytes": (C.c_size_t, [_i64, _i64, _i]),
    "dm4d_webp_encode_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp]),
    # baseline JPEG files decoded into a caller's buffer: speculative Huffman decoding, IDCT, up-sampling, colour (host/jpegdec.py)
    "dm4d_jpeg_decode_ws_bytes": (C.c_size_t, [_i64, _i]),
    "dm4d_jpeg_decode_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    # 8-bit PNG files decoded into a caller's buffer: inflate through an LDS window, then the unfilter wavefront (host/pngdec.py)
    "dm4d_png_decode_ws_bytes": (C.c_size_t, [_i64, _i]),
    "dm4d_png_decode_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp]),
    # raw captures: colour table + undistortion + area resize + crop of a batch of images, one launch (host/rectify.py)
    "dm4d_rectify_u8": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i64]),
}

# The constants of include/dm4d.h that the host uses, under the header's names without the DM4D_ prefix.  This block is their ONLY
# copy in Python (host/ops.py re-exports them); tests/test_abi.py reads the header and checks every value.
EPI_GEGLU = 1
EPI_SILU = 2
EPI_F32OUT = 4
EPI_F32SIDE = 8
EPI_SPLITOUT = 16
LOG2E = 1.4426950408889634
CAPTURE_FIELDS = 16
CAPTURE_CELL_FIELDS = 4
CAPTURE_PLANE_FIELDS = 8
CAPTURE_RECT_FIELDS = 8
EVAL_FIELDS = 16
EVAL_OUT = 8
EVAL_IMAGE_F32 = 1
EVAL_MASK_F32 = 2
EVAL_CROP_MASKS = 4
EVAL_BG_SHIFT = 3
LPIPS_TAPS = 5
LPIPS_IN_COLS = 64
VHULL_BLOCK = 256
VHULL_MAX_CHUNK = 1 << 26
TRIANG_MAX_VIEWS = 65536
SKEL_FIELDS = 8
SKEL_LINE = 0
SKEL_CIRCLE = 1
SKEL_MAX_PRIMS = 512
SKEL_COORD_MIN = -8192
SKEL_COORD_MAX = 8191
SKEL_MAX_SIZE = 16384
SKEL_MAX_KPTS = 2048
SKEL_LINK_FIELDS = 8
SKEL_ST_NONFINITE = 1
SKEL_ST_NOCOLOR = 2
SKEL_ST_LINK_SHIFT = 8
RESTORE_FIELDS = 16
JPEG_FIELDS = 8
JPEG_MCU_UNSTUFFED = 1248  # workspace bytes of unstuffed scan per 16 x 16 MCU
JPEG_MCU_BOUND = 2488      # bytes of stuffed scan per MCU, worst case
JPEG_CHUNK = 4096
POSE_FIELDS = 8
POSE_MAX_SIDE = 16384
POSE_MAX_HEATMAP_H = 4096
POSE_MAX_HEATMAP_W = 1024
POSE_TAB_LIMIT = 1 << 29
DETECT_MAX_ANCHORS = 1 << 20
DETECT_MAX_CLASSES = 4096
DETECT_MAX_KEEP = 256
DETECT_MAX_CANVAS = 4096
DETECT_COEF_ONE = 2048
MATTING_FIELDS = 8
MATTING_MAX_SIDE = 16384
PNG_FIELDS = 16
PNG_L = 0
PNG_RGBA = 1
PNG_STRIPE_BYTES = 32768
PNG_STRIPE_REC = 1712
WEBP_FIELDS = 8
WEBP_MAX_SIDE = 16383
WEBP_STRIPE_PIXELS = 8192
WEBP_STRIPE_REC = 3200
WEBP_IMAGE_REC = 4096
JPEGDEC_FIELDS = 16
JPEGDEC_TABLE_BYTES = 1104
JPEGDEC_SUB_BITS = 1024
JPEGDEC_TILE_LANES = 256
JPEGDEC_MAX_SCAN_BYTES = 1 << 28
JPEGDEC_ST_BAD_CODE = 1
JPEGDEC_ST_ZIGZAG = 2
JPEGDEC_ST_END = 4
JPEGDEC_ST_RANGE = 8
PNGDEC_FIELDS = 8
PNGDEC_RING_BYTES = 65536
PNGDEC_MAX_ROW_BYTES = 32768
PNGDEC_MAX_STREAM_BYTES = 1 << 28
PNGDEC_ST_HEADER = 1
PNGDEC_ST_BLOCK = 2
PNGDEC_ST_CODE = 4
PNGDEC_ST_DISTANCE = 8
PNGDEC_ST_END = 16
PNGDEC_ST_ADLER = 32
PNGDEC_ST_FILTER = 64
RECTIFY_FIELDS = 20
RECTIFY_MAX_SIDE = 16384
RECTIFY_MAX_SCALE = 8
ROWS_MOVE_MAX_JOBS = 16


class RowsMoveJob(C.Structure):
    """Dm4dRowsMoveJob of include/dm4d.h."""
    _fields_ = [("src", _vp), ("dst", _vp), ("src_row_idx", _vp), ("dst_row_idx", _vp), ("n_rows", _i64), ("row_bytes", _i64)]


class Dm4dError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def align16(n: int) -> int:
    """n rounded up to a multiple of 16: where the next region of a staging buffer or a workspace starts."""
    return (n + 15) // 16 * 16


def load():
    """Load libdm4d.so and attach prototypes.  Raises if it is missing -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise Dm4dError(
            f"{_LIB_PATH} not found: build the HIP extension first (python -m diffuman4d_amd.build). "
            "diffuman4d_amd has no CPU/PyTorch fallback path."
        )
    # PyTorch ships its own libamdhip64; load it FIRST so that libdm4d.so binds to the same HIP runtime instance as the
    # tensors and streams it is handed (loading libdm4d.so first pulls in /opt/rocm's copy and every launch then
    # fails with "no ROCm-capable device is detected")
    import torch  # noqa: F401
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().dm4d_last_error()
        raise Dm4dError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def hip_device(device, what: str):
    """`device` as a torch.device with an index, for the operator `what`; anything but an available HIP device is an error."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise Dm4dError(f"{what}: device {device!r} is not a HIP device (no CPU fallback in diffuman4d_amd)")
    if not torch.cuda.is_available():
        raise Dm4dError(f"{what}: no HIP device is available (no CPU fallback in diffuman4d_amd)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def call(name: str, *args) -> None:
    """Call the int-returning entry point `name`; a non-zero return raises Dm4dError under that same name."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        check(rc, name)
