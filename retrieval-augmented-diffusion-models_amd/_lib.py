"""ctypes binding of librdm_hip.so (include/rdm_hip.h) + a thin torch-tensor convenience layer.

There is deliberately NO fallback: if the shared library is missing this module raises at import,
and `Context()` raises when no HIP device is present.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RDM_HIP_LIB") or os.path.join(_HERE, "librdm_hip.so")   # env override: A/B builds (dev)

RDM_MAX_LEVELS = 8
ACT_NONE, ACT_GEGLU, ACT_QUICKGELU, ACT_SILU = 0, 1, 2, 3
PROF_CONV3X3, PROF_LINEAR, PROF_KNN, PROF_ATTENTION, PROF_GROUPNORM, PROF_LAYERNORM, PROF_UPSCONV = range(7)


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("model_channels", C.c_int),
                ("num_res_blocks", C.c_int), ("n_attention_resolutions", C.c_int),
                ("attention_resolutions", C.c_int * RDM_MAX_LEVELS), ("n_channel_mult", C.c_int),
                ("channel_mult", C.c_int * RDM_MAX_LEVELS), ("num_head_channels", C.c_int), ("context_dim", C.c_int)]


class VqCfg(C.Structure):
    _fields_ = [("embed_dim", C.c_int), ("n_embed", C.c_int), ("z_channels", C.c_int), ("ch", C.c_int),
                ("n_ch_mult", C.c_int), ("ch_mult", C.c_int * RDM_MAX_LEVELS), ("num_res_blocks", C.c_int),
                ("out_ch", C.c_int), ("resolution", C.c_int), ("mid_attn", C.c_int), ("kl", C.c_int),
                ("n_attn_resolutions", C.c_int), ("attn_resolutions", C.c_int * RDM_MAX_LEVELS)]


class RarmCfg(C.Structure):
    _fields_ = [("vocab_in", C.c_int), ("vocab_out", C.c_int), ("n_heads", C.c_int), ("d_head", C.c_int), ("depth", C.c_int),
                ("context_dim", C.c_int), ("sequence_length", C.c_int)]


class RarmSampleArgs(C.Structure):
    _fields_ = [("batch", C.c_int), ("k", C.c_int), ("cond_len", C.c_int), ("steps", C.c_int), ("temperature", C.c_float),
                ("top_k", C.c_int), ("guidance_scale", C.c_float)]


class LinearRowsForm(C.Structure):
    _fields_ = [("kernel", C.c_int), ("ma", C.c_int), ("nb", C.c_int), ("u", C.c_int), ("nw", C.c_int), ("ln", C.c_int), ("geglu", C.c_int)]


LINEAR_ROWS_REFUSED, LINEAR_ROWS_SGEMM, LINEAR_ROWS_MGEMM, LINEAR_ROWS_TILED = range(4)


class WgradForm(C.Structure):
    _fields_ = [("path", C.c_int), ("Z", C.c_int), ("per_plane", C.c_int), ("remap", C.c_int)]


WGRAD_PATHS = (None, "conv9<4>", "conv9<5>", "conv9<6>", "tn9", "tn1", "conv_fallback", "linear_fallback")


class ClipCfg(C.Structure):
    _fields_ = [("embed_dim", C.c_int), ("image_resolution", C.c_int), ("vision_layers", C.c_int),
                ("vision_width", C.c_int), ("vision_patch_size", C.c_int), ("context_length", C.c_int),
                ("vocab_size", C.c_int), ("transformer_width", C.c_int), ("transformer_heads", C.c_int),
                ("transformer_layers", C.c_int)]


class DdimArgs(C.Structure):
    _fields_ = [("S", C.c_int), ("batch", C.c_int), ("k", C.c_int), ("channels", C.c_int), ("height", C.c_int),
                ("width", C.c_int), ("eta", C.c_float), ("temperature", C.c_float),
                ("unconditional_guidance_scale", C.c_float), ("log_every_t", C.c_int), ("T", C.c_int),
                ("alphas_cumprod", C.POINTER(C.c_float))]


class DpmppArgs(C.Structure):
    _fields_ = [("batch", C.c_int), ("k", C.c_int), ("channels", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("unconditional_guidance_scale", C.c_float), ("order", C.c_int), ("lower_order_final", C.c_int),
                ("log_every_t", C.c_int), ("T", C.c_int), ("alphas_cumprod", C.POINTER(C.c_float)), ("n_nodes", C.c_int),
                ("nodes", C.POINTER(C.c_int))]


DPMPP_SKIP_TYPES = {"time_uniform": 0, "logSNR": 1}


class UnipcArgs(C.Structure):
    _fields_ = [("batch", C.c_int), ("k", C.c_int), ("channels", C.c_int), ("height", C.c_int), ("width", C.c_int),
                ("unconditional_guidance_scale", C.c_float), ("order", C.c_int), ("variant", C.c_int), ("corrector", C.c_int),
                ("lower_order_final", C.c_int), ("log_every_t", C.c_int), ("T", C.c_int), ("alphas_cumprod", C.POINTER(C.c_float)),
                ("n_nodes", C.c_int), ("nodes", C.POINTER(C.c_int))]


UNIPC_VARIANTS = {"bh1": 0, "bh2": 1}
UNIPC_COEFFICIENTS = ("alpha", "sigma", "a_x", "a_t", "a_1", "a_2", "a_3", "b_x", "b_0", "b_1", "b_2", "order_c", "order_p")
PLMS_STEP, PLMS_EULER_A, PLMS_EULER_B = 0, 1, 2          # rdm_op_plms_step's mode


class DdpmArgs(C.Structure):
    _fields_ = [("timesteps", C.c_int), ("batch", C.c_int), ("k", C.c_int), ("channels", C.c_int), ("height", C.c_int),
                ("width", C.c_int), ("clip_denoised", C.c_int), ("temperature", C.c_float), ("T", C.c_int),
                ("sqrt_recip_alphas_cumprod", C.POINTER(C.c_float)), ("sqrt_recipm1_alphas_cumprod", C.POINTER(C.c_float)),
                ("posterior_mean_coef1", C.POINTER(C.c_float)), ("posterior_mean_coef2", C.POINTER(C.c_float)),
                ("posterior_log_variance_clipped", C.POINTER(C.c_float))]


class Noise(C.Structure):
    """rdm_noise: a caller's stack, or the library's generator under (seed, row0); per_row and step are the step ops'."""
    _fields_ = [("stack", C.c_void_p), ("seeded", C.c_int), ("seed", C.c_uint64), ("row0", C.c_int64), ("per_row", C.c_int64),
                ("step", C.c_uint32)]


KNN_SCAN_PATHS = (None, "generic", "d512", "bulk")      # rdm_knn_form.path (RDM_KNN_SCAN_*)


class KnnForm(C.Structure):
    _fields_ = [("path", C.c_int), ("ksel", C.c_int), ("rescored", C.c_int), ("lists_per_block", C.c_int), ("queries_per_launch", C.c_int),
                ("eps", C.c_float)]


class KnnStages(C.Structure):
    _fields_ = [("rows_cap", C.c_int), ("nlists_cap", C.c_int), ("qn", C.c_void_p), ("qh", C.c_void_p), ("ql", C.c_void_p),
                ("cand_s", C.c_void_p), ("cand_i", C.c_void_p), ("flag", C.c_void_p), ("tau", C.c_void_p), ("tau_idx", C.c_void_p),
                ("theta", C.c_void_p), ("rows", C.c_int), ("nlists", C.c_int), ("form", KnnForm)]


_P = C.c_void_p
# name -> (restype, argtypes); exactly the symbols include/rdm_hip.h declares
SIGNATURES = {
    "rdm_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "rdm_ctx_destroy": (None, [_P]),
    "rdm_last_error": (C.c_char_p, [_P]),
    "rdm_set_stream": (C.c_int, [_P, _P]),
    "rdm_version": (C.c_char_p, []),
    "rdm_unet_manifest": (C.c_longlong, [C.POINTER(UNetCfg), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rdm_vq_manifest": (C.c_longlong, [C.POINTER(VqCfg), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rdm_clip_manifest": (C.c_longlong, [C.POINTER(ClipCfg), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rdm_load_unet": (C.c_int, [_P, C.POINTER(UNetCfg), _P, C.c_size_t]),
    "rdm_load_vq": (C.c_int, [_P, C.POINTER(VqCfg), _P, C.c_size_t]),
    "rdm_load_clip": (C.c_int, [_P, C.POINTER(ClipCfg), _P, C.c_size_t]),
    "rdm_rarm_manifest": (C.c_longlong, [C.POINTER(RarmCfg), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rdm_load_rarm": (C.c_int, [_P, C.POINTER(RarmCfg), _P, C.c_size_t]),
    "rdm_rarm_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "rdm_rarm_sample": (C.c_int, [_P, C.POINTER(RarmSampleArgs), _P, _P, _P, _P]),
    "rdm_rarm_sample_top_p": (C.c_int, [_P, C.POINTER(RarmSampleArgs), C.c_float, _P, _P, _P, _P]),
    "rdm_rarm_forward_seq": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "rdm_rarm_nll": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P]),
    "rdm_rarm_sample_prefill": (C.c_int, [_P, C.POINTER(RarmSampleArgs), C.c_float, _P, _P, _P, _P]),
    "rdm_vq_decode_indices": (C.c_int, [_P, _P, C.c_int, _P]),
    "rdm_unet_forward": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_ddim_num_intermediates": (C.c_int, [C.c_int, C.c_int]),
    "rdm_ddim_sample": (C.c_int, [_P, C.POINTER(DdimArgs), _P, _P, _P, C.POINTER(Noise), _P, _P, _P]),
    "rdm_plms_sample": (C.c_int, [_P, C.POINTER(DdimArgs), _P, _P, _P, _P, _P, _P]),
    "rdm_dpmpp_sample": (C.c_int, [_P, C.POINTER(DpmppArgs), _P, _P, _P, _P, _P, _P]),
    "rdm_dpmpp_timesteps": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "rdm_unipc_sample": (C.c_int, [_P, C.POINTER(UnipcArgs), _P, _P, _P, _P, _P, _P]),
    "rdm_unipc_coefficients": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(C.c_double)]),
    "rdm_ddpm_sample": (C.c_int, [_P, C.POINTER(DdpmArgs), _P, _P, C.POINTER(Noise), _P]),
    "rdm_rng_words": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "rdm_op_rng_words": (C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P]),
    "rdm_op_randn": (C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P]),
    "rdm_dpmpp_sde_sample": (C.c_int, [_P, C.POINTER(DpmppArgs), _P, _P, _P, C.POINTER(Noise), _P, _P, _P]),
    "rdm_unet_forward_guided": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_ddim_decode": (C.c_int, [_P, C.POINTER(DdimArgs), C.c_int, _P, _P, _P, C.POINTER(Noise), _P, _P, _P]),
    "rdm_ddim_encode": (C.c_int, [_P, C.POINTER(DdimArgs), C.c_int, _P, _P, _P, _P, _P]),
    "rdm_op_ddim_inverse_step": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    "rdm_op_q_sample_seeded": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_uint64, C.c_int64, _P]),
    "rdm_op_masked_blend": (C.c_int, [_P, _P, _P, _P, C.POINTER(Noise), C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P]),
    "rdm_ddim_inpaint": (C.c_int, [_P, C.POINTER(DdimArgs), C.c_int, _P, _P, _P, C.c_int, _P, _P, C.POINTER(Noise), _P, _P, _P, _P]),
    "rdm_vq_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "rdm_release_scratch": (C.c_int, [_P]),
    "rdm_vq_quantize": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "rdm_vq_decode_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rdm_vq_quantize_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "rdm_to_uint8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_clip_encode_text": (C.c_int, [_P, _P, C.c_int, _P]),
    "rdm_clip_encode_image": (C.c_int, [_P, _P, C.c_int, _P]),
    "rdm_clip_preprocess": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_clip_encode_image_raw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_db_load": (C.c_int, [_P, _P, C.c_longlong, C.c_int, C.c_int, C.c_int]),
    "rdm_db_size": (C.c_longlong, [_P]),
    "rdm_knn": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "rdm_knn_f64": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "rdm_knn_last_fallback": (C.c_int, [_P]),
    "rdm_db_gather": (C.c_int, [_P, _P, C.c_longlong, _P]),
    "rdm_knn_select": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(KnnForm)]),
    "rdm_op_knn_stages": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(KnnStages)]),
    "rdm_db_rows": (C.c_int, [_P, C.c_longlong, C.c_longlong, _P]),
    "rdm_knn_mask_words": (C.c_int, [C.c_longlong]),
    "rdm_knn_filtered": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "rdm_knn_filtered_f64": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "rdm_op_knn_stages_filtered": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.POINTER(KnnStages)]),
    "rdm_op_row_mask": (C.c_int, [_P, _P, C.c_longlong, C.c_longlong, C.c_int, _P]),
    "rdm_op_row_mask_count": (C.c_int, [_P, _P, C.c_int, C.c_longlong, _P]),
    "rdm_set_deterministic": (C.c_int, [_P, C.c_int]),
    "rdm_get_deterministic": (C.c_int, [_P]),
    "rdm_set_neighbour_bias": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "rdm_get_neighbour_bias": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rdm_op_xattn_fused_biased": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                            _P, _P, _P, _P]),
    "rdm_op_small_attention_biased": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_float, _P, C.c_int, _P]),
    "rdm_prof_enable": (C.c_int, [_P, C.c_int]),
    "rdm_prof_collect": (C.c_int, [_P, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rdm_prof_reset": (C.c_int, [_P]),
    "rdm_prof_dump": (C.c_int, [_P, C.c_char_p]),
    "rdm_debug_tap": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int]),
    "rdm_debug_guidance_prefix": (C.c_int, [_P, C.c_int]),
    "rdm_calib_probe": (C.c_int, [_P, _P, C.c_size_t, C.c_double, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rdm_comm_unique_id": (C.c_int, [_P, _P]),
    "rdm_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "rdm_comm_all_gather": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "rdm_comm_all_reduce_f32": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "rdm_comm_destroy": (C.c_int, [_P]),
    "rdm_vqenc_manifest": (C.c_longlong, [_P, _P, C.c_size_t, _P]),
    "rdm_load_vqenc": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "rdm_vq_encode": (C.c_int, [_P, _P, C.c_int, _P]),
    "rdm_vq_encode_hw": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_vq_encode_indices": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "rdm_op_q_sample": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_mse_loss": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_where_rows": (C.c_int, [_P, _P, _P, _P, _P, C.c_longlong, C.c_longlong]),
    "rdm_op_timestep_embedding": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "rdm_op_colsum_samples": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "rdm_op_expand2": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_linear": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "rdm_op_conv3x3": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int]),
    "rdm_op_conv3x3_down": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_vq_nearest_code": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_int, _P]),
    "rdm_op_moments_f64": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "rdm_op_knn_radius": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_manifold_hits": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "rdm_op_manifold_counts": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "rdm_op_nearest_d2": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "rdm_op_poly3_rowsums": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "rdm_op_rarm_sampler": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P]),
    "rdm_op_rarm_sampler_top_p": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, _P, _P, _P]),
    "rdm_op_conv3x3_dgrad": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_conv3x3_wgrad": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_groupnorm_bwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P, _P]),
    "rdm_op_layernorm_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P, _P, _P]),
    "rdm_op_groupnorm_bwd_add": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P, _P, _P, _P]),
    "rdm_op_layernorm_bwd_add": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P]),
    "rdm_op_colsum": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_int]),
    "rdm_op_transpose": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "rdm_op_add": (C.c_int, [_P, _P, _P, _P, C.c_longlong]),
    "rdm_op_dpmpp_step": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                    _P, _P, _P, _P]),
    "rdm_op_dpmpp_sde_step": (C.c_int, [_P, _P, _P, _P, C.POINTER(Noise), C.c_longlong, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_float, _P, _P, _P, _P]),
    "rdm_op_unipc_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.POINTER(C.c_double), _P, _P, _P, _P, _P]),
    "rdm_op_ddim_step": (C.c_int, [_P, _P, _P, C.POINTER(Noise), C.c_longlong, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, _P, _P, _P]),
    "rdm_op_plms_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                   C.c_int, _P, _P, _P, _P]),
    "rdm_op_ddpm_step": (C.c_int, [_P, _P, _P, C.POINTER(Noise), C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                   C.c_int, C.c_float, _P]),
    "rdm_op_geglu": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int]),
    "rdm_op_linear_ln": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "rdm_op_linear_wgrad": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int, C.c_int]),
    "rdm_op_ema": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_float]),
    "rdm_op_silu": (C.c_int, [_P, _P, _P, _P, C.c_longlong]),
    "rdm_op_sumpool2": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_adamw": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "rdm_op_attention_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rdm_op_bmm": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]),
    "rdm_op_heads": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_transpose_batched": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "rdm_op_softmax": (C.c_int, [_P, _P, _P, C.c_longlong, C.c_int, C.c_int]),
    "rdm_op_softmax_bwd": (C.c_int, [_P, _P, _P, _P, C.c_longlong, C.c_int]),
    "rdm_op_groupnorm": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_float, C.c_int, _P]),
    "rdm_op_layernorm": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_float, _P]),
    "rdm_op_layernorm_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_float, _P]),
    "rdm_op_linear_res_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_self_attention": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_self_attention_qkv": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_head_conv": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_conv_in": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_conv_out": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_linear_rowvec": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int]),
    "rdm_op_xattn_fused_ln3": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rdm_op_xattn_fused": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_causal_attention_d64": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int, _P, _P, C.c_int]),
    "rdm_op_rarm_nll": (C.c_int, [_P, _P, C.c_longlong, C.c_int, _P, _P]),
    "rdm_linear_rows_select": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LinearRowsForm)]),
    "rdm_op_linear_rows": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_wgrad_select": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(WgradForm)]),
    "rdm_op_rarm_decode_attention": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_float, _P,
                                               C.c_int, C.c_int, C.c_int]),
    "rdm_op_rarm_xattn_decode": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rdm_op_rarm_embed": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rdm_op_vq_attention": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int]),
    "rdm_op_causal_attention_d64_bwd": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int]),
    "rdm_op_rarm_nll_bwd": (C.c_int, [_P, _P, C.c_longlong, C.c_int, _P, C.c_float, _P, _P]),
    "rdm_op_embedding_grad": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "rdm_op_small_attention": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_float, _P, C.c_int]),
    "rdm_op_adamw_multi": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "rdm_op_ema_multi": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_float]),
    "rdm_op_small_attention_bwd": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P]),
}


def load_library(path: str = LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"librdm_hip.so not found at {path}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C retrieval-augmented-diffusion-models_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


lib = load_library()


def linear_rows_select(M, N, K, act=ACT_NONE, ln=False, deterministic=False):
    """The kernel Context.op_linear_rows launches for this shape (host only, no device): a tuple ("sgemm", MA, NB, U, NW, LN, GEGLU) with
    the skinny kernel's instantiation, ("mgemm",), ("tiled",), or ("refused",) where the LayerNorm-in-kernel form declines the shape."""
    f = LinearRowsForm()
    rc = lib.rdm_linear_rows_select(int(M), int(N), int(K), int(act), int(bool(ln)), int(bool(deterministic)), C.byref(f))
    if rc != 0:
        raise RdmError(f"rdm_linear_rows_select({M}, {N}, {K}, act={act}, ln={ln}, deterministic={deterministic}) failed ({rc})")
    if f.kernel == LINEAR_ROWS_SGEMM:
        return ("sgemm", f.ma, f.nb, f.u, f.nw, bool(f.ln), bool(f.geglu))
    return (("refused", "sgemm", "mgemm", "tiled")[f.kernel],)


def wgrad_select(*shape):
    """The kernel Context.op_conv3x3_wgrad (shape = (B, H, W, C, N)) or Context.op_linear_wgrad (shape = (M, N, K)) launches (host only, no
    device): (path, Z, per_plane, remap) with path one of WGRAD_PATHS -- "conv9<4|5|6>" the nine-tap kernel at width 16 / 32 / 64, "tn9" /
    "tn1" the per-tap kernel, the two transposed-copy fallbacks; Z planes of per_plane chunks / rows / K' positions; remap as in rdm_hip.h."""
    f = WgradForm()
    if len(shape) == 5:
        B, H, W, Cc, N = (int(v) for v in shape)
        rc = lib.rdm_wgrad_select(1, B, H, W, Cc, N, 0, 0, C.byref(f))
    elif len(shape) == 3:
        M, N, K = (int(v) for v in shape)
        rc = lib.rdm_wgrad_select(0, 0, 0, 0, 0, N, M, K, C.byref(f))
    else:
        raise RdmError(f"wgrad_select takes (B, H, W, C, N) or (M, N, K), got {shape}")
    if rc != 0:
        raise RdmError(f"rdm_wgrad_select{shape} failed ({rc})")
    return (WGRAD_PATHS[f.path], f.Z, f.per_plane, f.remap)


def knn_select(n, dim, b, k):
    """What Context.knn does for a database of n rows x dim, b queries, k neighbours (host only, no device): a dict with path (one of
    KNN_SCAN_PATHS), ksel, rescored, lists_per_block, queries_per_launch and eps, the score-error bound of the certificate."""
    f = KnnForm()
    if lib.rdm_knn_select(int(n), int(dim), int(b), int(k), C.byref(f)) != 0:
        raise RdmError(f"rdm_knn_select(n={n}, dim={dim}, b={b}, k={k}): arguments the search refuses")
    return {"path": KNN_SCAN_PATHS[f.path], "ksel": f.ksel, "rescored": f.rescored, "lists_per_block": f.lists_per_block,
            "queries_per_launch": f.queries_per_launch, "eps": float(f.eps)}


NO_ROW = 0xffffffff          # the index a filtered search returns where a mask allows fewer than k rows (its score is -inf)


def knn_mask_words(n):
    """64-bit words of one row mask for a database of n rows: n rounded up to the scans' 256-row tile, / 64 (rdm_knn_mask_words)."""
    return int(lib.rdm_knn_mask_words(int(n)))


def pack_row_mask(allowed):
    """Host packer: bool [n] -> int64 [knn_mask_words(n)] holding the uint64 words of the mask, bit r % 64 of word r / 64 = allowed[r]."""
    a = np.asarray(allowed)
    if a.dtype != np.bool_ or a.ndim != 1 or a.shape[0] < 1:
        raise RdmError(f"pack_row_mask: a boolean array of length n >= 1, got {a.dtype} {a.shape}")
    bits = np.zeros(knn_mask_words(a.shape[0]) * 64, dtype=np.bool_)
    bits[:a.shape[0]] = a
    return np.packbits(bits, bitorder="little").view(np.uint64).view(np.int64).copy()


def shard_row_mask(rows, row0, n_local):
    """The local index list of the shard holding the global rows [row0, row0 + n_local): rows (int array, or bool array over the whole
    database) -> sorted int64 local indices.  row0 need not be a multiple of 64: every shard builds its own mask from local indices."""
    r = np.asarray(rows)
    if r.dtype == np.bool_:
        r = np.flatnonzero(r)
    if r.ndim != 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
        raise RdmError(f"shard_row_mask: rows must be a 1-d integer or boolean array, got {r.dtype} {r.shape}")
    r = r.astype(np.int64)
    if (r < 0).any():
        raise RdmError("shard_row_mask: negative row index")
    r = r[(r >= row0) & (r < row0 + n_local)] - int(row0)
    return np.unique(r)


def row_filter_args(allow, mask_of_query, b, words):
    """Checks of Context.knn's filter arguments that need no device -> (allow as [n_masks, words], n_masks, int32 ids or None)."""
    if allow is None:
        if mask_of_query is not None:
            raise RdmError("knn: mask_of_query needs allow")
        return None, 0, None
    if not isinstance(allow, torch.Tensor) or allow.dtype != torch.int64:
        raise RdmError("knn: allow must be an int64 tensor holding the masks' 64-bit words (Context.row_mask / pack_row_mask)")
    if allow.ndim == 1:
        allow = allow[None]
    if allow.ndim != 2 or allow.shape[1] != words or allow.shape[0] < 1:
        raise RdmError(f"knn: allow must be [n_masks, {words}] for this database, got {tuple(allow.shape)}")
    n_masks = int(allow.shape[0])
    ids = None
    if mask_of_query is not None:
        ids = np.ascontiguousarray(mask_of_query.cpu().numpy() if isinstance(mask_of_query, torch.Tensor) else mask_of_query)
        if ids.shape != (b,) or not np.issubdtype(ids.dtype, np.integer):
            raise RdmError(f"knn: mask_of_query must hold one integer per query ([{b}]), got {ids.dtype} {ids.shape}")
        bad = np.flatnonzero((ids < 0) | (ids >= n_masks))
        if bad.size:
            raise RdmError(f"knn: query {int(bad[0])} names mask {int(ids[bad[0]])}: mask_of_query must lie in [0, {n_masks})")
        ids = ids.astype(np.int32)
    return allow, n_masks, ids


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous(), "tensor must be contiguous"
        return C.c_void_p(t.data_ptr())
    raise TypeError(type(t))


def make_unet_cfg(in_channels=3, out_channels=3, model_channels=192, num_res_blocks=2, attention_resolutions=(8, 4, 2),
                  channel_mult=(1, 2, 3, 5), num_head_channels=32, context_dim=512, **other) -> UNetCfg:
    """UNetModel keyword arguments (openaimodel.py:228-262) -> rdm_unet_cfg.  Arguments that do not change the sampling graph are
    accepted and dropped; ones that select a graph the library does not build raise instead of being silently ignored."""
    inert = {"image_size", "use_checkpoint", "use_fp16", "dropout", "legacy", "use_new_attention_order", "num_heads", "num_heads_upsample"}
    required = {"conv_resample": True, "dims": 2, "num_classes": None, "use_scale_shift_norm": False, "resblock_updown": False,
                "use_spatial_transformer": True, "transformer_depth": 1, "n_embed": None}
    for k_, v_ in other.items():
        if k_ in inert:
            continue
        if k_ not in required:
            raise TypeError(f"make_unet_cfg: unknown UNetModel argument {k_!r}")
        if v_ != required[k_]:
            raise NotImplementedError(f"UNetModel({k_}={v_!r}): the native graph is built for {k_}={required[k_]!r} (every shipped RDM config)")
    c = UNetCfg()
    c.in_channels, c.out_channels, c.model_channels, c.num_res_blocks = in_channels, out_channels, model_channels, num_res_blocks
    c.n_attention_resolutions = len(attention_resolutions)
    for i, v in enumerate(attention_resolutions):
        c.attention_resolutions[i] = int(v)
    c.n_channel_mult = len(channel_mult)
    for i, v in enumerate(channel_mult):
        c.channel_mult[i] = int(v)
    c.num_head_channels, c.context_dim = num_head_channels, context_dim
    return c


def make_vq_cfg(embed_dim=3, n_embed=8192, z_channels=3, ch=128, ch_mult=(1, 2, 4), num_res_blocks=2, out_ch=3,
                resolution=256, mid_attn=True, kl=False, attn_resolutions=(), **_ignored) -> VqCfg:
    c = VqCfg()
    c.embed_dim, c.n_embed, c.z_channels, c.ch = embed_dim, n_embed, z_channels, ch
    c.n_ch_mult = len(ch_mult)
    for i, v in enumerate(ch_mult):
        c.ch_mult[i] = int(v)
    c.num_res_blocks, c.out_ch, c.resolution, c.mid_attn, c.kl = num_res_blocks, out_ch, resolution, int(mid_attn), int(kl)
    c.n_attn_resolutions = len(attn_resolutions)
    for i, v in enumerate(attn_resolutions):
        c.attn_resolutions[i] = int(v)
    return c


def make_vqgan_f16_cfg(**kw) -> VqCfg:
    """taming VQModel of the RARM models (models/rarm/imagenet/dogs/config.yaml:28-51)."""
    d = dict(embed_dim=256, n_embed=16384, z_channels=256, ch=128, ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2, out_ch=3, resolution=256,
             attn_resolutions=(16,))
    d.update(kw)
    return make_vq_cfg(**d)


def make_rarm_cfg(in_channels=16386, out_channels=16384, n_heads=12, d_head=64, depth=18, context_dim=512, sequence_length=256,
                  **other) -> RarmCfg:
    """RetrievalPatchTransformer params (models/rarm/imagenet/dogs/config.yaml:14-27; rdm/modules/attention.py:206-220).  The native
    graph is the shipped one: token input (continuous=False), learned positions, causal self-attention + cross-attention to the
    neighbours, no outer residual; anything else raises instead of being silently ignored."""
    required = {"positional_encodings": True, "cross_attend": True, "causal": True, "continuous": False, "residual": False}
    for k_, v_ in other.items():
        if k_ in ("dropout", "checkpoint"):
            continue
        if k_ not in required:
            raise TypeError(f"make_rarm_cfg: unknown RetrievalPatchTransformer argument {k_!r}")
        if v_ != required[k_]:
            raise NotImplementedError(f"RetrievalPatchTransformer({k_}={v_!r}): the native graph is built for {k_}={required[k_]!r}")
    return RarmCfg(vocab_in=in_channels, vocab_out=out_channels, n_heads=n_heads, d_head=d_head, depth=depth, context_dim=context_dim,
                   sequence_length=sequence_length)


def make_clip_cfg(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32,
                  context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                  transformer_layers=12, **_ignored) -> ClipCfg:
    c = ClipCfg()
    (c.embed_dim, c.image_resolution, c.vision_layers, c.vision_width, c.vision_patch_size, c.context_length,
     c.vocab_size, c.transformer_width, c.transformer_heads, c.transformer_layers) = (
        embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
        transformer_width, transformer_heads, transformer_layers)
    return c


def manifest_text(kind: str, cfg):
    """-> (the manifest as the library writes it: one "offset nbytes kind src,src,..." line per entry, blob_bytes)"""
    fn = {"unet": lib.rdm_unet_manifest, "vq": lib.rdm_vq_manifest, "vqenc": lib.rdm_vqenc_manifest, "clip": lib.rdm_clip_manifest,
          "rarm": lib.rdm_rarm_manifest}[kind]
    blob = C.c_size_t(0)
    n = fn(C.byref(cfg), None, 0, C.byref(blob))
    if n < 0:
        raise ValueError(f"unsupported {kind} config")
    buf = C.create_string_buffer(int(n) + 1)
    fn(C.byref(cfg), buf, int(n) + 1, C.byref(blob))
    return buf.value.decode(), int(blob.value)


def manifest(kind: str, cfg):
    """-> (list of (offset, nbytes, kind, [src...]), blob_bytes)"""
    text, blob_bytes = manifest_text(kind, cfg)
    out = []
    for line in text.splitlines():
        off, nb, kd, srcs = line.split(" ")
        out.append((int(off), int(nb), kd, srcs.split(",")))
    return out, blob_bytes


class RdmError(RuntimeError):
    pass


def check_top_p(what, top_p):
    """The nucleus mass of the RARM sampler: None or 1.0 -> None (no nucleus filter, the entry without one); a number in (0, 1) -> float."""
    if top_p is None:
        return None
    try:
        v = float(top_p)
    except (TypeError, ValueError):
        raise RdmError(f"{what}: top_p must be a number in (0, 1], got {top_p!r}") from None
    if not (0.0 < v <= 1.0):                                   # NaN fails both comparisons
        raise RdmError(f"{what}: top_p must lie in (0, 1], got {top_p!r}")
    return None if v == 1.0 else v


def _acp_array(alphas_cumprod):
    return np.ascontiguousarray(alphas_cumprod.detach().cpu().numpy() if isinstance(alphas_cumprod, torch.Tensor) else alphas_cumprod,
                                dtype=np.float32)


def _nodes_array(nodes):
    return np.ascontiguousarray(np.asarray(nodes).reshape(-1), dtype=np.int32)


def dpmpp_timesteps(S, alphas_cumprod, skip_type="logSNR"):
    """Node list for Context.dpmpp_sample (rdm_dpmpp_timesteps; host code, no context needed): "time_uniform" = DDIM's S-step
    timesteps descending, then 0; "logSNR" = uniform in logSNR from T - 1 to 0, rounded to integer timesteps (may come out shorter
    than S steps when targets collide).  -> int32 numpy array, strictly decreasing, ending in 0."""
    if skip_type not in DPMPP_SKIP_TYPES:
        raise RdmError(f"dpmpp_timesteps: skip_type must be one of {sorted(DPMPP_SKIP_TYPES)}, got {skip_type!r}")
    ac = _acp_array(alphas_cumprod)
    T, S = ac.shape[0], int(S)
    out = np.empty((max(S, len(range(0, T, max(T // max(S, 1), 1)))) + 1,), dtype=np.int32)
    n = lib.rdm_dpmpp_timesteps(ac.ctypes.data_as(C.POINTER(C.c_float)), T, S, DPMPP_SKIP_TYPES[skip_type],
                                out.ctypes.data_as(C.POINTER(C.c_int)))
    if n < 2:
        raise RdmError(f"dpmpp_timesteps: bad arguments (S={S}, T={T}, skip_type={skip_type!r})")
    return out[:n].copy()


def rng_words(seed, row, step, stream, block):
    """The four Philox4x32-10 words of one block of the library's noise generator (rdm_rng_words; host code, no context needed): key =
    the 64-bit seed, counter = (block, step, row, stream).  -> uint32 numpy array [4]."""
    out = np.zeros((4,), dtype=np.uint32)
    if lib.rdm_rng_words(int(seed) & (2 ** 64 - 1), int(row), int(step), int(stream), int(block), out.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise RdmError("rng_words: bad arguments")
    return out


def _noise_seed(what, seed, row0, B):
    """The (seed, row0) of a device-noise call, checked before any pointer crosses the ABI: the seed modulo 2^64, rows [row0, row0 + B)
    32-bit counters."""
    row0 = int(row0)
    if row0 < 0 or row0 + int(B) >= 2 ** 32:
        raise RdmError(f"{what}: rows [row0, row0 + B) must be non-negative and row0 + B must fit 32 bits, got row0={row0}, B={int(B)}")
    return int(seed) & (2 ** 64 - 1), row0


def _noise_source(ctx, what, x_T, cond, noise, seed, row0, shape=None):
    """Where a sampling call's step noise comes from -> (Noise, stack, x_shape).  Without a seed: the caller's stack on ctx's device (or
    None; the struct points into it), x_shape None.  With one: no stack may be given (refused before ctx is touched); x_shape is the call's
    latent shape (x_T's, or cond's rows at `shape` -- what sizes a call without x_T) and (seed, row0) are validated for its rows."""
    if seed is None:
        stack = None if noise is None else ctx._dev(noise, torch.float32)
        return Noise(stack=_ptr(stack)), stack, None
    if noise is not None:
        raise RdmError(f"{what}: give a seed or a noise stack, not both")
    x_shape = Context._seeded_shape(what, x_T, cond, shape)
    seed, row0 = _noise_seed(what, seed, row0, x_shape[0])
    return Noise(seeded=1, seed=seed, row0=row0), None, x_shape


def _unipc_variant(what, variant):
    if variant not in UNIPC_VARIANTS:
        raise RdmError(f"{what}: variant must be one of {sorted(UNIPC_VARIANTS)}, got {variant!r}")
    return UNIPC_VARIANTS[variant]


def unipc_coefficients(nodes, alphas_cumprod, j, order=2, variant="bh2", corrector=True, lower_order_final=True):
    """The float64 scalars of the UniPC pass after forward j over `nodes` (rdm_unipc_coefficients; host code, no context needed):
    -> float64 numpy array [13] in the order of UNIPC_COEFFICIENTS: alpha_j, sigma_j, the correction x_j = a_x x_{j-1} + a_t m_j +
    a_1 m_{j-1} + a_2 m_{j-2} + a_3 m_{j-3} (order_c 0: x_j = u_j), the prediction u_{j+1} = b_x x_j + b_0 m_j + b_1 m_{j-1} + b_2 m_{j-2}."""
    ac = _acp_array(alphas_cumprod)
    nd = _nodes_array(nodes)
    out = np.zeros((len(UNIPC_COEFFICIENTS),), dtype=np.float64)
    r = lib.rdm_unipc_coefficients(ac.ctypes.data_as(C.POINTER(C.c_float)), ac.shape[0], nd.ctypes.data_as(C.POINTER(C.c_int)), nd.shape[0],
                                   int(j), int(order), _unipc_variant("unipc_coefficients", variant), int(bool(corrector)),
                                   int(bool(lower_order_final)), out.ctypes.data_as(C.POINTER(C.c_double)))
    if r != 0:
        raise RdmError(f"unipc_coefficients: bad arguments (j={j}, order={order}, {nd.shape[0]} nodes: strictly decreasing timesteps in "
                       f"[0, {ac.shape[0] - 1}], 0 <= j <= n_nodes - 2, order 1 | 2 | 3)")
    return out


class Context:
    """One library context per HIP device (include/rdm_hip.h: rdm_ctx)."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise RdmError("rdm_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        h = _P()
        rc = lib.rdm_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise RdmError(f"rdm_ctx_create failed ({rc}); no usable HIP device {device}")
        self._h = h
        self.device = torch.device("cuda", device)
        self.unet_cfg = self.vq_cfg = self.vqenc_cfg = self.clip_cfg = self.rarm_cfg = None
        self.comm_world = 0                   # ranks of the context's RCCL communicator (comm_init), 0 = none

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "comm_world", 0):
                try:
                    self.comm_destroy()
                except Exception:
                    pass
            lib.rdm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RdmError(f"librdm_hip error {rc}: {lib.rdm_last_error(self._h).decode()}")

    def release_scratch(self):
        """Hand the grow-only work buffers (training scratch, split-K planes, ...) back to the allocator; re-created on demand."""
        self._check(lib.rdm_release_scratch(self._h))

    def use_current_stream(self):
        self._check(lib.rdm_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    # ---- weights
    def load_unet(self, cfg: UNetCfg, blob: np.ndarray):
        self._check(lib.rdm_load_unet(self._h, C.byref(cfg), blob.ctypes.data_as(_P), blob.nbytes)); self.unet_cfg = cfg

    def load_vq(self, cfg: VqCfg, blob: np.ndarray):
        self._check(lib.rdm_load_vq(self._h, C.byref(cfg), blob.ctypes.data_as(_P), blob.nbytes)); self.vq_cfg = cfg

    def load_vq_encoder(self, cfg: VqCfg, blob: np.ndarray):
        """First-stage ENCODER weights (`encoder.*`, `quant_conv.*` of the first-stage state dict; packing.pack("vqenc", cfg, sd))."""
        self._check(lib.rdm_load_vqenc(self._h, C.byref(cfg), blob.ctypes.data_as(_P), blob.nbytes)); self.vqenc_cfg = cfg

    def vq_encode(self, img):
        """VQModelInterface.encode: image f32 [b,out_ch,H,W] in [-1,1], H and W multiples of f = 2^(levels-1) -> latent f32
        [b,embed_dim,H/f,W/f] (not quantised).  The encoder is conv-only, so any such size runs (rdm_vq_encode_hw); a first stage with a
        wide latent (VQGAN-f16) runs at its own resolution only."""
        img = self._dev(img, torch.float32)
        cfg = self._need("vq_encode", "vqenc")
        f = 1 << (cfg.n_ch_mult - 1)
        if img.ndim != 4 or img.shape[1] != cfg.out_ch:
            raise RdmError(f"vq_encode: image must be [b,{cfg.out_ch},H,W], got {tuple(img.shape)}")
        b, _, H, W = img.shape
        if b < 1 or H < f or W < f or H % f or W % f:
            raise RdmError(f"vq_encode: image height and width must be positive multiples of {f}, got {tuple(img.shape)}")
        if cfg.embed_dim > 4 and (H, W) != (cfg.resolution, cfg.resolution):
            raise RdmError(f"vq_encode: a first stage with a wide latent takes [b,{cfg.out_ch},{cfg.resolution},{cfg.resolution}] only, got {tuple(img.shape)}")
        z = torch.empty((b, cfg.embed_dim, H // f, W // f), device=self.device, dtype=torch.float32)
        if cfg.embed_dim > 4:
            self._check(lib.rdm_vq_encode(self._h, _ptr(img), b, _ptr(z)))
        else:
            self._check(lib.rdm_vq_encode_hw(self._h, _ptr(img), b, H, W, _ptr(z)))
        return z

    def vq_encode_indices(self, img, return_quant=False):
        """taming VQModel.encode as Net2NetTransformer.encode_to_z reaches it: image f32 [b,out_ch,R,R] in [-1,1] -> code indices
        int64 [b, h*w] (nearest codebook row of quant_conv(encoder(x)), first minimum on ties); return_quant: -> (quant f32
        [b,embed_dim,h,w] = the chosen codebook rows, indices).  Needs the encoder AND the decoder (it holds the codebook) of a
        first stage with a wide latent (VQGAN-f16)."""
        img = self._dev(img, torch.float32)
        cfg = self._need("vq_encode_indices", "vqenc")
        self._need("vq_encode_indices", "vq")
        if img.ndim != 4 or tuple(img.shape[1:]) != (cfg.out_ch, cfg.resolution, cfg.resolution):
            raise RdmError(f"vq_encode_indices: image must be [b,{cfg.out_ch},{cfg.resolution},{cfg.resolution}], got {tuple(img.shape)}")
        b = img.shape[0]
        if b < 1:
            raise RdmError("vq_encode_indices: empty batch")
        zr = cfg.resolution >> (cfg.n_ch_mult - 1)
        idx = torch.empty((b, zr * zr), device=self.device, dtype=torch.int64)
        quant = torch.empty((b, cfg.embed_dim, zr, zr), device=self.device, dtype=torch.float32) if return_quant else None
        self._check(lib.rdm_vq_encode_indices(self._h, _ptr(img), b, _ptr(idx), _ptr(quant)))
        return (quant, idx) if return_quant else idx

    def vq_nearest_code(self, z, codebook):
        """The nearest-code kernel alone: z f32 [M, E], codebook f32 [N, E] -> int32 [M] = argmin_j |e_j|^2 - 2 z . e_j in fp32, first
        minimum on ties.  E: multiples of 64 up to 512 (the library rejects others)."""
        z = self._dev(z, torch.float32); codebook = self._dev(codebook, torch.float32)
        if z.ndim != 2 or codebook.ndim != 2 or z.shape[1] != codebook.shape[1] or z.shape[0] < 1 or codebook.shape[0] < 1:
            raise RdmError(f"vq_nearest_code: z must be [M,E] and codebook [N,E], got {tuple(z.shape)} and {tuple(codebook.shape)}")
        out = torch.empty((z.shape[0],), device=self.device, dtype=torch.int32)
        self._check(lib.rdm_op_vq_nearest_code(self._h, _ptr(z), _ptr(codebook), z.shape[0], codebook.shape[0], z.shape[1], _ptr(out)))
        return out

    # ---- quality metrics on feature sets (csrc/metrics.hip; rdm_amd.metrics holds the host arithmetic)
    def _features(self, what, x, name="x"):
        """A feature set f32 [n, d] on the device.  The row count and d are checked by the library (it names the op and the value)."""
        if not isinstance(x, torch.Tensor) or x.ndim != 2:
            raise RdmError(f"{what}: {name} must be a tensor [n, d], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        return self._dev(x, torch.float32)

    def op_moments_f64(self, x, sum_, outer):
        """sum_ f64 [d] += SUM_i x_i, outer f64 [d, d] += SUM_i x_i x_i^T in fp64 (rdm_op_moments_f64): in / out, both on this device,
        zeroed by the caller before the first batch.  x f32 [n, d], d % 32 == 0, 32 <= d <= 4096."""
        x = self._features("op_moments_f64", x)
        d = x.shape[1]
        for name, t, shape in (("sum_", sum_, (d,)), ("outer", outer, (d, d))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous():
                raise RdmError(f"op_moments_f64: {name} must be a contiguous float64 tensor {shape} on {self.device} (it is accumulated into)")
        self._check(lib.rdm_op_moments_f64(self._h, _ptr(x), x.shape[0], d, _ptr(sum_), _ptr(outer)))

    def op_knn_radius(self, x, k):
        """-> f32 [n]: squared Euclidean distance from each row of x f32 [n, d] to its k-th nearest OTHER row (rdm_op_knn_radius; self is
        left out by index, duplicates are neighbours at 0).  1 <= k <= 8, k < n."""
        x = self._features("op_knn_radius", x)
        out = torch.empty((x.shape[0],), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_knn_radius(self._h, _ptr(x), x.shape[0], x.shape[1], int(k), _ptr(out)))
        return out

    def op_manifold_hits(self, probe, ref, ref_radius2):
        """-> uint8 [m]: 1 iff probe row i lies within ref_radius2[j] (squared) of some row j of ref (rdm_op_manifold_hits).
        probe f32 [m, d], ref f32 [n, d], ref_radius2 f32 [n]."""
        probe = self._features("op_manifold_hits", probe, "probe"); ref = self._features("op_manifold_hits", ref, "ref")
        if probe.shape[1] != ref.shape[1]:
            raise RdmError(f"op_manifold_hits: probe and ref must share d, got {tuple(probe.shape)} and {tuple(ref.shape)}")
        if not isinstance(ref_radius2, torch.Tensor) or tuple(ref_radius2.shape) != (ref.shape[0],):
            raise RdmError(f"op_manifold_hits: ref_radius2 must be a tensor [{ref.shape[0]}], one radius per ref row")
        ref_radius2 = self._dev(ref_radius2, torch.float32)
        out = torch.empty((probe.shape[0],), device=self.device, dtype=torch.uint8)
        self._check(lib.rdm_op_manifold_hits(self._h, _ptr(probe), probe.shape[0], _ptr(ref), _ptr(ref_radius2), ref.shape[0], ref.shape[1], _ptr(out)))
        return out

    def op_manifold_counts(self, probe, ref, ref_radius2):
        """-> int32 [m]: the number of rows j of ref with probe row i within ref_radius2[j] (squared) of them (rdm_op_manifold_counts):
        op_manifold_hits that counts where it ORs.  probe f32 [m, d], ref f32 [n, d], ref_radius2 f32 [n]."""
        probe = self._features("op_manifold_counts", probe, "probe"); ref = self._features("op_manifold_counts", ref, "ref")
        if probe.shape[1] != ref.shape[1]:
            raise RdmError(f"op_manifold_counts: probe and ref must share d, got {tuple(probe.shape)} and {tuple(ref.shape)}")
        if not isinstance(ref_radius2, torch.Tensor) or tuple(ref_radius2.shape) != (ref.shape[0],):
            raise RdmError(f"op_manifold_counts: ref_radius2 must be a tensor [{ref.shape[0]}], one radius per ref row")
        ref_radius2 = self._dev(ref_radius2, torch.float32)
        out = torch.empty((probe.shape[0],), device=self.device, dtype=torch.int32)
        self._check(lib.rdm_op_manifold_counts(self._h, _ptr(probe), probe.shape[0], _ptr(ref), _ptr(ref_radius2), ref.shape[0], ref.shape[1], _ptr(out)))
        return out

    def op_nearest_d2(self, probe, ref):
        """-> f32 [m]: the squared Euclidean distance from probe row i to the nearest row of ref, nothing left out (rdm_op_nearest_d2).
        probe f32 [m, d], ref f32 [n, d]."""
        probe = self._features("op_nearest_d2", probe, "probe"); ref = self._features("op_nearest_d2", ref, "ref")
        if probe.shape[1] != ref.shape[1]:
            raise RdmError(f"op_nearest_d2: probe and ref must share d, got {tuple(probe.shape)} and {tuple(ref.shape)}")
        out = torch.empty((probe.shape[0],), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_nearest_d2(self._h, _ptr(probe), probe.shape[0], _ptr(ref), ref.shape[0], ref.shape[1], _ptr(out)))
        return out

    def op_poly3_rowsums(self, probe, ref, gamma, coef0=1.0, exclude_same_index=False, out=None):
        """-> f64 [G, m] (or [m] for 2-D arguments, one group): entry (g, i) = SUM_j (gamma probe[g, i] . ref[g, j] + coef0)^3 over the rows
        of ref's group g, without j == i when exclude_same_index (rdm_op_poly3_rowsums): dot product in fp32, the rest in fp64.
        probe f32 [G, m, d] and ref f32 [G, n, d], or [m, d] and [n, d].  out: optional contiguous float64 tensor of the result's shape on
        this device, written and returned."""
        for name, x in (("probe", probe), ("ref", ref)):
            if not isinstance(x, torch.Tensor) or x.ndim not in (2, 3):
                raise RdmError(f"op_poly3_rowsums: {name} must be a tensor [G, rows, d] or [rows, d], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        if probe.ndim != ref.ndim:
            raise RdmError(f"op_poly3_rowsums: probe and ref must both be 3-D or both 2-D, got {tuple(probe.shape)} and {tuple(ref.shape)}")
        flat = probe.ndim == 2
        p3 = self._dev(probe[None] if flat else probe, torch.float32); r3 = self._dev(ref[None] if flat else ref, torch.float32)
        if p3.shape[0] != r3.shape[0]:
            raise RdmError(f"op_poly3_rowsums: probe has {p3.shape[0]} groups and ref {r3.shape[0]}; group g's probes see group g's refs")
        if p3.shape[2] != r3.shape[2]:
            raise RdmError(f"op_poly3_rowsums: probe and ref must share d, got {tuple(probe.shape)} and {tuple(ref.shape)}")
        shape = (p3.shape[1],) if flat else (p3.shape[0], p3.shape[1])
        if out is None:
            out = torch.empty(shape, device=self.device, dtype=torch.float64)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != shape or out.device != self.device or not out.is_contiguous():
            raise RdmError(f"op_poly3_rowsums: out must be a contiguous float64 tensor {shape} on {self.device}")
        self._check(lib.rdm_op_poly3_rowsums(self._h, _ptr(p3), p3.shape[1], _ptr(r3), r3.shape[1], p3.shape[2], p3.shape[0],
                                             int(bool(exclude_same_index)), float(gamma), float(coef0), _ptr(out)))
        return out

    def load_clip(self, cfg: ClipCfg, blob: np.ndarray):
        self._check(lib.rdm_load_clip(self._h, C.byref(cfg), blob.ctypes.data_as(_P), blob.nbytes)); self.clip_cfg = cfg

    def load_rarm(self, cfg: RarmCfg, blob: np.ndarray):
        self._check(lib.rdm_load_rarm(self._h, C.byref(cfg), blob.ctypes.data_as(_P), blob.nbytes)); self.rarm_cfg = cfg

    # ---- RARM
    def _check_rarm(self, what, context, b):
        if self.rarm_cfg is None:
            raise RdmError(f"{what}: rarm weights not loaded")
        if context.ndim != 3 or context.shape[0] != b or context.shape[2] != self.rarm_cfg.context_dim:
            raise RdmError(f"{what}: neighbours must be [b={b},k,{self.rarm_cfg.context_dim}], got {tuple(context.shape)}")

    def _check_ids(self, what, ids, n, name):
        """nn.Embedding / get_codebook_entry raise IndexError on an id outside the table; the kernels would silently read row 0.
        One tiny reduction + a host read per call (not per token)."""
        if ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= n:
                raise RdmError(f"{what}: {name} must lie in [0, {n}), got values in [{lo}, {hi}]")

    def rarm_forward(self, tokens, context):
        """RetrievalPatchTransformer.forward: tokens int64 [b,t], context f32 [b,k,ctx] -> logits f32 [b,t,vocab_out]."""
        tokens = self._dev(tokens, torch.int64); context = self._dev(context, torch.float32)
        b, t = tokens.shape
        self._check_rarm("rarm_forward", context, b)
        self._check_ids("rarm_forward", tokens, self.rarm_cfg.vocab_in, "tokens")
        out = torch.empty((b, t, self.rarm_cfg.vocab_out), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_rarm_forward(self._h, _ptr(tokens), b, t, _ptr(context), context.shape[1], _ptr(out)))
        return out

    RARM_SEQ_MAX_K = 128      # neighbours per sequence of the whole-sequence entries (small_attention's LDS limit)

    def _check_rarm_seq(self, what, tokens, context):
        b, t = tokens.shape
        self._check_rarm(what, context, b)
        self._check_ids(what, tokens, self.rarm_cfg.vocab_in, "tokens")
        if t < 1 or t > self.rarm_cfg.sequence_length:
            raise RdmError(f"{what}: {t} positions exceed the positional encoding (sequence_length {self.rarm_cfg.sequence_length})")
        if context.shape[1] > self.RARM_SEQ_MAX_K:
            raise RdmError(f"{what}: at most {self.RARM_SEQ_MAX_K} neighbours per sequence, got k={context.shape[1]}")
        return b, t

    def rarm_forward_seq(self, tokens, context):
        """rarm_forward in ONE pass over all positions (include/rdm_hip.h rdm_rarm_forward_seq): -> logits f32 [b,t,vocab_out]."""
        tokens = self._dev(tokens, torch.int64); context = self._dev(context, torch.float32)
        if self.rarm_cfg is None:
            raise RdmError("rarm_forward_seq: rarm weights not loaded")
        b, t = self._check_rarm_seq("rarm_forward_seq", tokens, context)
        out = torch.empty((b, t, self.rarm_cfg.vocab_out), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_rarm_forward_seq(self._h, _ptr(tokens), b, t, _ptr(context), context.shape[1], _ptr(out)))
        return out

    def rarm_nll(self, tokens, targets, context):
        """F.cross_entropy(RetrievalPatchTransformer.forward(tokens, context), targets, reduction='none') without the [b,t,vocab] logits
        (rdm_rarm_nll): tokens, targets int64 [b,t] -> f32 [b,t]."""
        tokens = self._dev(tokens, torch.int64); targets = self._dev(targets, torch.int64); context = self._dev(context, torch.float32)
        if self.rarm_cfg is None:
            raise RdmError("rarm_nll: rarm weights not loaded")
        b, t = self._check_rarm_seq("rarm_nll", tokens, context)
        if tuple(targets.shape) != (b, t):
            raise RdmError(f"rarm_nll: targets must be [{b},{t}], got {tuple(targets.shape)}")
        self._check_ids("rarm_nll", targets, self.rarm_cfg.vocab_out, "targets")
        out = torch.empty((b, t), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_rarm_nll(self._h, _ptr(tokens), _ptr(targets), b, t, _ptr(context), context.shape[1], _ptr(out)))
        return out

    def rarm_sample(self, cond_tokens, context, steps, uniforms, temperature=1.0, top_k=None, guidance_scale=1.0, top_p=None, prefill=False):
        """LatentImageRETRO.sample with sample=True: -> tokens int64 [b,steps].  uniforms f32 [steps,b] in [0,1).
        top_p in (0, 1]: nucleus filter after top-k (include/rdm_hip.h rdm_rarm_sample_top_p); None or 1.0: none, today's entry.
        prefill: the conditioning prefix runs in one whole-sequence pass instead of token by token (rdm_rarm_sample_prefill)."""
        top_p = check_top_p("rarm_sample", top_p)
        cond_tokens = self._dev(cond_tokens, torch.int64); context = self._dev(context, torch.float32)
        uniforms = self._dev(uniforms, torch.float32)
        b, tc = cond_tokens.shape
        self._check_rarm("rarm_sample", context, b)
        self._check_ids("rarm_sample", cond_tokens, self.rarm_cfg.vocab_in, "cond_tokens")
        if tuple(uniforms.shape) != (steps, b):
            raise RdmError(f"rarm_sample: uniforms must be [{steps},{b}], got {tuple(uniforms.shape)}")
        a = RarmSampleArgs(batch=b, k=context.shape[1], cond_len=tc, steps=steps, temperature=temperature,
                           top_k=int(top_k) if top_k is not None else 0, guidance_scale=guidance_scale)
        out = torch.empty((b, steps), device=self.device, dtype=torch.int64)
        if prefill:
            if tc + steps - 1 > self.rarm_cfg.sequence_length:
                raise RdmError(f"rarm_sample: {tc + steps - 1} positions exceed the positional encoding (sequence_length {self.rarm_cfg.sequence_length})")
            if context.shape[1] > self.RARM_SEQ_MAX_K:
                raise RdmError(f"rarm_sample: prefill takes at most {self.RARM_SEQ_MAX_K} neighbours per sequence, got k={context.shape[1]}")
            self._check(lib.rdm_rarm_sample_prefill(self._h, C.byref(a), 1.0 if top_p is None else top_p, _ptr(cond_tokens), _ptr(context),
                                                    _ptr(uniforms), _ptr(out)))
        elif top_p is None:
            self._check(lib.rdm_rarm_sample(self._h, C.byref(a), _ptr(cond_tokens), _ptr(context), _ptr(uniforms), _ptr(out)))
        else:
            self._check(lib.rdm_rarm_sample_top_p(self._h, C.byref(a), top_p, _ptr(cond_tokens), _ptr(context), _ptr(uniforms), _ptr(out)))
        return out

    def vq_decode_indices(self, indices):
        """decode_to_img: code indices int64 [b, h*w] -> image f32 [b,out_ch,R,R] (VQGAN first stage with a wide latent)."""
        indices = self._dev(indices, torch.int64)
        self._need("vq_decode_indices", "vq")
        zr = self.vq_cfg.resolution >> (self.vq_cfg.n_ch_mult - 1)
        if indices.ndim != 2 or indices.shape[1] != zr * zr:
            raise RdmError(f"vq_decode_indices: indices must be [b,{zr * zr}], got {tuple(indices.shape)}")
        self._check_ids("vq_decode_indices", indices, self.vq_cfg.n_embed, "indices")
        img = torch.empty((indices.shape[0], self.vq_cfg.out_ch, self.vq_cfg.resolution, self.vq_cfg.resolution), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_vq_decode_indices(self._h, _ptr(indices), indices.shape[0], _ptr(img)))
        return img

    # ---- model calls (torch CUDA tensors in / out)
    def _dev(self, t, dtype):
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _need(self, what, name):
        """The binding sizes its outputs from the loaded configuration: fail like the C ABI does (a message, not an AttributeError)."""
        cfg = getattr(self, name + "_cfg")
        if cfg is None:
            raise RdmError(f"{what}: {name} weights not loaded (load_{name})")
        return cfg

    def _check_sampler_shapes(self, what, x, cond, uncond=None, noise=None, steps=None):
        """The C ABI takes raw pointers: reject every shape it would silently mis-read (the reference raises a torch
        shape error in the same situations, e.g. `torch.cat([c, uc])` in ddim.py:232 for an unconditional conditioning of
        the wrong rank)."""
        if self.unet_cfg is None:
            raise RdmError(f"{what}: unet weights not loaded")
        cd, cin = self.unet_cfg.context_dim, self.unet_cfg.in_channels
        if x.ndim != 4 or x.shape[1] != cin:
            raise RdmError(f"{what}: latent must be [B,{cin},H,W], got {tuple(x.shape)}")
        if cond.ndim != 3 or cond.shape[0] != x.shape[0] or cond.shape[2] != cd or cond.shape[1] < 1:
            raise RdmError(f"{what}: conditioning must be [B={x.shape[0]},k,{cd}], got {tuple(cond.shape)}")
        if uncond is not None and tuple(uncond.shape) != tuple(cond.shape):
            raise RdmError(f"{what}: unconditional conditioning {tuple(uncond.shape)} must match the conditioning {tuple(cond.shape)}")
        if noise is not None and tuple(noise.shape) != (steps,) + tuple(x.shape):
            raise RdmError(f"{what}: noise stack must be {(steps,) + tuple(x.shape)}, got {tuple(noise.shape)}")

    def unet_forward(self, x, t, context):
        x = self._dev(x, torch.float32); t = self._dev(t, torch.int64); context = self._dev(context, torch.float32)
        self._check_sampler_shapes("unet_forward", x, context)
        if t.ndim != 1 or t.shape[0] != x.shape[0]:
            raise RdmError(f"unet_forward: timesteps must be [B={x.shape[0]}], got {tuple(t.shape)}")
        b, _, H, W = x.shape
        out = torch.empty((b, self.unet_cfg.out_channels, H, W), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_unet_forward(self._h, _ptr(x), _ptr(t), _ptr(context), b, context.shape[1], H, W, _ptr(out)))
        return out

    def unet_forward_guided(self, x, t, cond, uncond):
        """rdm_unet_forward_guided: the UNet on [x | x] against [cond | uncond] at the one timestep t, through the kernel configurations
        the sampling loops run it in (shared prefix of the doubled batch, zero-context shortcut, time-embedding table) -> eps
        [2B, Cout, H, W], rows cond | uncond."""
        x, cond, uncond = (self._dev(v, torch.float32) for v in (x, cond, uncond))
        self._check_sampler_shapes("unet_forward_guided", x, cond, uncond)
        b, _, H, W = x.shape
        out = torch.empty((2 * b, self.unet_cfg.out_channels, H, W), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_unet_forward_guided(self._h, _ptr(x), int(t), _ptr(cond), _ptr(uncond), b, cond.shape[1], H, W, _ptr(out)))
        return out

    def _sampler_call(self, what, fn, Args, x_T, cond, uncond, alphas_cumprod, scale, log_every_t, want_intermediates, S=None, nodes=None,
                      noise=None, nz=None, x_shape=None, run_steps=None, want_pred_x0=True, **fields):
        """What ddim_sample, plms_sample, dpmpp_sample and unipc_sample share: device casts, the fp32 alphas_cumprod array, the step
        count (of DDIM's S-step schedule, or of the node list), shape and guidance checks, the outputs.  Args(**fields) plus the fields
        every sampler has is the argument struct, fn(handle, args, x_T, cond, uncond, [nz,] z, x_inter, pred_x0_inter) the library call;
        nz: the Noise of a sampler that takes one; noise: a [steps, B, C, H, W] stack to shape-check; x_shape: the latent shape of a
        seeded call without x_T (fn then gets a null x_T and the library draws the start); run_steps: the steps a decode / encode call
        runs of the S-step schedule, in [1, its length] -- what then sizes the noise stack and the intermediates; want_pred_x0 False: no
        pred_x0_inter is allocated (fn gets null: the inversion logs x only).  -> (z, x_inter, pred_x0_inter)."""
        x_T, cond, uncond = (None if t is None else self._dev(t, torch.float32) for t in (x_T, cond, uncond))
        x_arg = x_T
        if x_T is None:
            x_T = torch.empty(tuple(int(v) for v in x_shape), device="meta", dtype=torch.float32)     # shapes only
        ac = _acp_array(alphas_cumprod)
        if nodes is None:
            steps = len(range(0, ac.shape[0], max(ac.shape[0] // max(int(S), 1), 1)))
            fields["S"] = S
        else:
            nd = _nodes_array(nodes)
            steps = nd.shape[0] - 1
            fields.update(n_nodes=nd.shape[0], nodes=nd.ctypes.data_as(C.POINTER(C.c_int)))
        if run_steps is not None:
            if not 1 <= int(run_steps) <= steps:
                raise RdmError(f"{what}: the step count must lie in [1, {steps}] (the schedule of S={S}), got {run_steps}")
            steps = int(run_steps)
        self._check_sampler_shapes(what, x_T, cond, uncond, noise, steps)
        if scale > 1.0 and uncond is None:
            raise RdmError(f"{what}: unconditional_conditioning is required when unconditional_guidance_scale > 1")
        B, Cc, H, W = x_T.shape
        a = Args(batch=B, k=cond.shape[1], channels=Cc, height=H, width=W, unconditional_guidance_scale=scale, log_every_t=log_every_t,
                 T=ac.shape[0], alphas_cumprod=ac.ctypes.data_as(C.POINTER(C.c_float)), **fields)
        z = torch.empty(tuple(x_T.shape), device=self.device, dtype=torch.float32)
        xi = pi = None
        if want_intermediates:
            n = lib.rdm_ddim_num_intermediates(steps, log_every_t)
            xi = torch.empty((n,) + tuple(x_T.shape), device=self.device, dtype=torch.float32)
            pi = torch.empty_like(xi) if want_pred_x0 else None
        self._check(fn(self._h, C.byref(a), _ptr(x_arg), _ptr(cond), _ptr(uncond), *([] if nz is None else [C.byref(nz)]), _ptr(z), _ptr(xi),
                       _ptr(pi)))
        return z, xi, pi

    def ddim_sample(self, S, x_T, cond, uncond, alphas_cumprod, eta=0.0, scale=1.0, noise=None, log_every_t=100,
                    temperature=1.0, want_intermediates=False, seed=None, row0=0, shape=None):
        """rdm_ddim_sample; with `seed` step i's noise is the library's own (seed, stream 1, step i, row0 + b),
        generated in the step kernel (no stack; `noise` must then be None), and x_T may be None -- the start is then drawn from stream 0
        at the latent `shape` (C, H, W), for cond.shape[0] rows."""
        if seed is None and x_T is None:
            raise RdmError("ddim_sample: x_T is required without a seed")
        nz, noise, x_shape = _noise_source(self, "ddim_sample", x_T, cond, noise, seed, row0, shape)
        return self._sampler_call("ddim_sample", lib.rdm_ddim_sample, DdimArgs, x_T, cond, uncond, alphas_cumprod, scale, log_every_t,
                                  want_intermediates, S=S, nz=nz, noise=noise if eta != 0.0 else None,   # (its shape matters only when it is used)
                                  x_shape=x_shape, eta=eta, temperature=temperature)

    def ddim_decode(self, S, t_start, x_latent, cond, uncond, alphas_cumprod, eta=0.0, scale=1.0, noise=None, log_every_t=100,
                    temperature=1.0, want_intermediates=False, seed=None, row0=0):
        """rdm_ddim_decode (ldm DDIMSampler.decode): the DDIM loop of the S-step schedule from x_latent at level index t_start - 1 down
        to index 0, t_start forwards; t_start = the schedule's length is ddim_sample.  noise: a [t_start, B, C, H, W] stack for
        eta > 0; with `seed` step i of this call takes the library's (seed, stream 1, step i, row0 + b), and
        `noise` must be None.  Returns (z, x_inter, pred_x0_inter); the intermediates are None unless want_intermediates."""
        if x_latent is None:
            raise RdmError("ddim_decode: x_latent is required")
        t_start = int(t_start)
        nz, noise, _ = _noise_source(self, "ddim_decode", x_latent, cond, noise, seed, row0)
        return self._sampler_call("ddim_decode", lambda h, a, *rest: lib.rdm_ddim_decode(h, a, t_start, *rest), DdimArgs, x_latent, cond, uncond,
                                  alphas_cumprod, scale, log_every_t, want_intermediates, S=S, nz=nz, noise=noise if eta != 0.0 else None,
                                  run_steps=t_start, eta=eta, temperature=temperature)

    @staticmethod
    def _blend_mask(what, mask, shape):
        """The mask of a blend over a latent of `shape` (B, C, H, W): [B, 1, H, W] or [B, C, H, W] -> its channel count."""
        B, Cc, H, W = (int(v) for v in shape)
        if mask.ndim != 4 or tuple(mask.shape) not in ((B, 1, H, W), (B, Cc, H, W)):
            raise RdmError(f"{what}: mask must be [{B},1,{H},{W}] or [{B},{Cc},{H},{W}], got {tuple(mask.shape)}")
        return int(mask.shape[1])

    def ddim_inpaint(self, S, t_start, x_latent, x0, mask, cond, uncond, alphas_cumprod, eta=0.0, scale=1.0, noise=None, q_noise=None,
                     log_every_t=100, temperature=1.0, want_intermediates=False, seed=None, row0=0):
        """rdm_ddim_inpaint: ddim_decode's loop with the inpainting blend before every forward -- at loop step i the iterate becomes
        (sqrt(a) x0 + sqrt(1 - a) z_i) mask + (1 - mask) x at that step's level a; mask [B, 1 | C, H, W] in [0, 1], 1 = keep the known
        latent x0.  z_i = q_noise[i], q_noise a [t_start, B, C, H, W] stack (required without a seed); noise: the update noise stack for
        eta > 0, as ddim_decode's.  With `seed` no stack of either kind -- the update noise is the library's
        (seed, stream 1, step i), the known region's (seed, stream 0, step i + 1), rows row0 + b.  The result of the last step is not
        blended.  Returns (z, x_inter, pred_x0_inter); the intermediates are None unless want_intermediates."""
        if x_latent is None or x0 is None or mask is None:
            raise RdmError("ddim_inpaint: x_latent, x0 and mask are required")
        t_start = int(t_start)
        if seed is not None and q_noise is not None:
            raise RdmError("ddim_inpaint: give a seed or a q_noise stack, not both")
        nz, noise, _ = _noise_source(self, "ddim_inpaint", x_latent, cond, noise, seed, row0)
        x0, mask = self._dev(x0, torch.float32), self._dev(mask, torch.float32)
        if tuple(x0.shape) != tuple(x_latent.shape):
            raise RdmError(f"ddim_inpaint: x0 {tuple(x0.shape)} must have the latent's shape {tuple(x_latent.shape)}")
        mc = self._blend_mask("ddim_inpaint", mask, x_latent.shape)
        if seed is None:
            if q_noise is None:
                raise RdmError("ddim_inpaint: a q_noise stack [t_start, B, C, H, W] is required without a seed")
            q_noise = self._dev(q_noise, torch.float32)
            if tuple(q_noise.shape) != (t_start,) + tuple(x_latent.shape):
                raise RdmError(f"ddim_inpaint: q_noise must be {(t_start,) + tuple(x_latent.shape)}, got {tuple(q_noise.shape)}")
        fn = lambda h, a, x, c, u, n, *out: lib.rdm_ddim_inpaint(h, a, t_start, x, _ptr(x0), _ptr(mask), mc, c, u, n, _ptr(q_noise), *out)
        return self._sampler_call("ddim_inpaint", fn, DdimArgs, x_latent, cond, uncond, alphas_cumprod, scale, log_every_t, want_intermediates,
                                  S=S, nz=nz, noise=noise if eta != 0.0 else None, run_steps=t_start, eta=eta, temperature=temperature)

    def op_masked_blend(self, x, x0, mask, z, sqrt_a, sqrt_1ma, out=None, x_dup=None, seed=None, row0=0, step=1):
        """The inpainting blend kernel alone on caller-owned contiguous fp32 device tensors: out = (sqrt_a x0 + sqrt_1ma z) mask +
        (1 - mask) x over x [B, C, H, W], mask [B, 1 | C, H, W] (1 = x0), z of x's size or None (zeros) (rdm_op_masked_blend).  With `seed`
        (and no z) z is the library's (seed, stream 0, step, row0 + b), drawn in the kernel -- step i + 1 for
        loop step i; C * H * W must then be a multiple of 4 and x, x0, out, x_dup 16-byte aligned.  out (default: a new tensor) may be x;
        x_dup receives the same values.  -> out."""
        ok = lambda t: t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
        if x.ndim != 4 or not all(ok(t) for t in (x, x0, mask)):
            raise RdmError("op_masked_blend: x [B, C, H, W], x0 and mask must be contiguous fp32 device tensors")
        if tuple(x0.shape) != tuple(x.shape):
            raise RdmError(f"op_masked_blend: x0 {tuple(x0.shape)} must have x's shape {tuple(x.shape)}")
        mc = self._blend_mask("op_masked_blend", mask, x.shape)
        if out is None:
            out = torch.empty_like(x)
        for t in (z, out, x_dup):
            if t is not None and (not ok(t) or t.numel() != x.numel()):
                raise RdmError("op_masked_blend: z, out and x_dup must be contiguous fp32 device tensors of x's size")
        B, Cc, H, W = (int(v) for v in x.shape)
        nz = Noise(stack=_ptr(z))
        if seed is not None:
            if z is not None:
                raise RdmError("op_masked_blend: a seeded call takes no z operand")
            step = int(step)
            if not 0 <= step < 2 ** 32:
                raise RdmError(f"op_masked_blend: step is a 32-bit counter, got {step}")
            seed, row0 = _noise_seed("op_masked_blend", seed, row0, B)
            nz = Noise(seeded=1, seed=seed, row0=row0, step=step)
        self._check(lib.rdm_op_masked_blend(self._h, _ptr(x), _ptr(x0), _ptr(mask), C.byref(nz), B, Cc, H, W, mc, float(sqrt_a), float(sqrt_1ma),
                                            _ptr(out), _ptr(x_dup)))
        return out

    def ddim_encode(self, S, t_enc, x0, cond, uncond, alphas_cumprod, scale=1.0, log_every_t=100, want_intermediates=False, eta=0.0):
        """rdm_ddim_encode: deterministic DDIM inversion of x0, t_enc steps up the S-step schedule with the UNet at each step's target
        timestep; the result is at level index t_enc - 1, what ddim_decode(t_start=t_enc) expects.  scale: the inversion's own guidance
        scale.  eta is there to be refused: it must be 0.  Returns (z, x_inter): the iterate after the steps the rule
        i % log_every_t == 0 or i == t_enc - 1 logs, None unless want_intermediates."""
        if x0 is None:
            raise RdmError("ddim_encode: x0 is required")
        if eta != 0.0:
            raise RdmError(f"ddim_encode: eta must be 0 (the inversion is deterministic), got {eta}")
        t_enc = int(t_enc)
        z, xi, _ = self._sampler_call("ddim_encode", lambda h, a, x, c, u, z, xi, pi: lib.rdm_ddim_encode(h, a, t_enc, x, c, u, z, xi),
                                      DdimArgs, x0, cond, uncond, alphas_cumprod, scale, log_every_t, want_intermediates, S=S,
                                      run_steps=t_enc, want_pred_x0=False, eta=0.0, temperature=1.0)
        return z, xi

    def op_ddim_inverse_step(self, x, eps, cfg, scale, sqrt_a_cur, sqrt_one_minus_a_cur, sqrt_a_next, sqrt_one_minus_a_next, x_out, x_dup=None,
                             pred_x0=None):
        """The DDIM inversion step kernel alone on caller-owned fp32 device tensors of x.numel() elements (eps: twice that under cfg,
        [cond | uncond]): pred_x0 = (x - sqrt_one_minus_a_cur e) / sqrt_a_cur, x_out = sqrt_a_next pred_x0 + sqrt_one_minus_a_next e.
        x_out may be x; x_dup / pred_x0 may be None.  Writes into the given outputs."""
        n = self._step_sizes("op_ddim_inverse_step", x, eps, cfg, (x_out, x_dup, pred_x0))
        self._check(lib.rdm_op_ddim_inverse_step(self._h, _ptr(x), _ptr(eps), n, int(bool(cfg)), float(scale), float(sqrt_a_cur),
                                                 float(sqrt_one_minus_a_cur), float(sqrt_a_next), float(sqrt_one_minus_a_next), _ptr(x_out),
                                                 _ptr(x_dup), _ptr(pred_x0)))

    def op_q_sample_seeded(self, x0, sqrt_a, sqrt_1ma, seed, row0=0, out=None):
        """sqrt_a x0 + sqrt_1ma z on x0 [B, ...] (fp32, device), z the library's starting-latent normals (seed, stream 0, step 0,
        row0 + b) drawn in the pass that applies them: no noise tensor (rdm_op_q_sample_seeded).  The elements per row must be a
        multiple of 4 and x0 / out 16-byte aligned.  out: a tensor of x0's size to write into (may be x0)."""
        if x0.ndim < 2 or x0.dtype != torch.float32 or not x0.is_cuda or not x0.is_contiguous():
            raise RdmError("op_q_sample_seeded: x0 must be a contiguous fp32 device tensor [B, ...]")
        B, per_row = int(x0.shape[0]), int(x0[0].numel())
        seed, row0 = _noise_seed("op_q_sample_seeded", seed, row0, B)
        if out is None:
            out = torch.empty_like(x0)
        elif out.dtype != torch.float32 or out.numel() != x0.numel() or not out.is_cuda or not out.is_contiguous():
            raise RdmError("op_q_sample_seeded: out must be a contiguous fp32 device tensor of x0's size")
        self._check(lib.rdm_op_q_sample_seeded(self._h, _ptr(x0), B, per_row, float(sqrt_a), float(sqrt_1ma), seed, row0, _ptr(out)))
        return out

    @staticmethod
    def _seeded_shape(what, x_T, cond, shape):
        """(B, C, H, W) of a seeded sampling call: x_T's, or cond's rows at the given latent shape (C, H, W)."""
        if x_T is not None:
            return tuple(x_T.shape)
        if shape is None or len(tuple(shape)) != 3:
            raise RdmError(f"{what}: a seeded call without x_T needs the latent shape (C, H, W)")
        return (int(cond.shape[0]),) + tuple(int(v) for v in shape)

    def _rng_fill(self, what, fn, dtype, seed, B, per_row, row0, step, stream, out):
        B, per_row, step, stream = int(B), int(per_row), int(step), int(stream)
        if B < 1 or per_row < 1:
            raise RdmError(f"{what}: B and per_row must be >= 1, got B={B}, per_row={per_row}")
        if not (0 <= step < 2 ** 32 and 0 <= stream < 2 ** 32):
            raise RdmError(f"{what}: step and stream are 32-bit counters, got step={step}, stream={stream}")
        seed, row0 = _noise_seed(what, seed, row0, B)
        if out is None:
            out = torch.empty((B, per_row), device=self.device, dtype=dtype)
        elif out.dtype != dtype or out.numel() != B * per_row or not out.is_cuda:
            raise RdmError(f"{what}: out must be a {dtype} device tensor of B * per_row = {B * per_row} elements")
        self._check(fn(self._h, seed, row0, B, per_row, step, stream, _ptr(out)))
        return out

    def op_rng_words(self, seed, B, per_row, row0=0, step=0, stream=0, out=None):
        """The Philox word each element of rows row0 .. row0 + B - 1 consumes at (step, stream): int32 [B, per_row] holding the uint32 bits
        (rdm_op_rng_words; include/rdm_hip.h "device noise").  out: an int32 device tensor of B * per_row elements to write into."""
        return self._rng_fill("op_rng_words", lib.rdm_op_rng_words, torch.int32, seed, B, per_row, row0, step, stream, out)

    def op_randn(self, seed, B, per_row, row0=0, step=0, stream=0, out=None):
        """The library's normals: f32 [B, per_row], row b element e a function of (seed, stream, step, row0 + b, e) only (rdm_op_randn).
        stream 0 / step 0 is the starting latent of the seeded samplers, stream 1 / step i the update noise of loop step i."""
        return self._rng_fill("op_randn", lib.rdm_op_randn, torch.float32, seed, B, per_row, row0, step, stream, out)

    def plms_sample(self, S, x_T, cond, uncond, alphas_cumprod, scale=1.0, log_every_t=100, want_intermediates=False):
        """ldm PLMSSampler's loop (eta = 0) on DDIM's schedule: S' + 1 UNet forwards for S' sampler timesteps.  Returns
        (z, x_inter, pred_x0_inter); the intermediates are None unless want_intermediates."""
        return self._sampler_call("plms_sample", lib.rdm_plms_sample, DdimArgs, x_T, cond, uncond, alphas_cumprod, scale, log_every_t,
                                  want_intermediates, S=S, eta=0.0, temperature=1.0)

    @staticmethod
    def _step_sizes(what, x, eps, cfg, others, name="x"):
        """What the step-kernel bindings check before a pointer crosses the ABI: eps holds x.numel() elements (twice that under cfg) and
        every other operand given x.numel().  name: what the binding calls x."""
        n = x.numel()
        if eps.numel() != (2 * n if cfg else n) or any(t is not None and t.numel() != n for t in others):
            raise RdmError(f"{what}: operand sizes do not match {name}")
        return n

    @staticmethod
    def _step_noise(what, noise, n, seed, row0, per_row, step):
        """The Noise of a step-kernel call: the noise operand (or None), or, with a seed, (seed, row0, per_row, step); the library checks
        that per_row divides n."""
        if seed is None:
            return Noise(stack=_ptr(noise))
        if noise is not None or per_row is None:
            raise RdmError(f"{what}: a seeded call takes per_row and no noise operand")
        per_row, step = int(per_row), int(step)
        if per_row < 1 or not 0 <= step < 2 ** 32:
            raise RdmError(f"{what}: per_row must be >= 1 and step a 32-bit counter, got per_row={per_row}, step={step}")
        seed, row0 = _noise_seed(what, seed, row0, max(n // per_row, 1))
        return Noise(seeded=1, seed=seed, row0=row0, per_row=per_row, step=step)

    def op_ddim_step(self, x, eps, noise, cfg, scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, temperature, x_prev, x_dup=None, pred_x0=None,
                     seed=None, row0=0, per_row=None, step=0):
        """The DDIM update kernel alone on caller-owned fp32 device tensors of x.numel() elements (eps: twice that under cfg,
        [cond | uncond]) with the kernel's own scalars (rdm_op_ddim_step); noise / x_dup / pred_x0 may be None, x_prev may be x.  With
        `seed` (and no noise) the noise of (seed, stream 1, step, row0 + b) for rows of per_row elements, drawn
        in the kernel.  Writes into the given outputs."""
        n = self._step_sizes("op_ddim_step", x, eps, cfg, (noise, x_prev, x_dup, pred_x0))
        sc = [float(v) for v in (scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, temperature)]
        nz = self._step_noise("op_ddim_step", noise, n, seed, row0, per_row, step)
        self._check(lib.rdm_op_ddim_step(self._h, _ptr(x), _ptr(eps), C.byref(nz), n, int(bool(cfg)), *sc, _ptr(x_prev), _ptr(x_dup),
                                         _ptr(pred_x0)))

    def op_plms_step(self, x, eps, cfg, scale, a_t, a_prev, sqrt_one_minus_at, mode, order, x_out, e_prev=None, h1=None, h2=None, h3=None,
                     e_store=None, x_dup=None, pred_x0=None):
        """The PLMS update kernel alone on caller-owned fp32 device tensors of x.numel() elements (eps: twice that under cfg,
        [cond | uncond]); mode PLMS_STEP (with `order` history operands h1 .. h3) | PLMS_EULER_A | PLMS_EULER_B (with e_prev); e_store
        receives the guided e_t in the first two modes and may be h3; x_out may be x.  Writes into the given outputs."""
        n = self._step_sizes("op_plms_step", x, eps, cfg, (e_prev, h1, h2, h3, e_store, x_out, x_dup, pred_x0))
        self._check(lib.rdm_op_plms_step(self._h, _ptr(x), _ptr(eps), _ptr(e_prev), _ptr(h1), _ptr(h2), _ptr(h3), n, int(bool(cfg)),
                                         float(scale), float(a_t), float(a_prev), float(sqrt_one_minus_at), int(mode), int(order),
                                         _ptr(e_store), _ptr(x_out), _ptr(x_dup), _ptr(pred_x0)))

    def op_ddpm_step(self, x, eps, noise, sqrt_recip, sqrt_recipm1, coef1, coef2, log_var, clip, nonzero, temperature, x_prev, seed=None,
                     row0=0, per_row=None, step=0):
        """The ancestral DDPM update kernel alone on caller-owned fp32 device tensors of x.numel() elements (rdm_op_ddpm_step); noise may
        be None when nonzero is false, x_prev may be x.  With `seed` (and no noise) the library's noise, as op_ddim_step.  Writes
        into x_prev."""
        n = self._step_sizes("op_ddpm_step", x, eps, False, (noise, x_prev))
        sc = [float(v) for v in (sqrt_recip, sqrt_recipm1, coef1, coef2, log_var)]
        nz = self._step_noise("op_ddpm_step", noise, n, seed, row0, per_row, step)
        self._check(lib.rdm_op_ddpm_step(self._h, _ptr(x), _ptr(eps), C.byref(nz), n, *sc, int(bool(clip)), int(bool(nonzero)),
                                         float(temperature), _ptr(x_prev)))

    @staticmethod
    def dpmpp_timesteps(S, alphas_cumprod, skip_type="logSNR"):
        return dpmpp_timesteps(S, alphas_cumprod, skip_type)

    def dpmpp_sample(self, nodes, x_T, cond, uncond, alphas_cumprod, scale=1.0, order=2, lower_order_final=None, log_every_t=100,
                     want_intermediates=False):
        """DPM-Solver++(2M) (order 1: DDIM with eta = 0) over the strictly decreasing integer timesteps `nodes` (dpmpp_timesteps builds
        the two grids): len(nodes) - 1 UNet forwards, the result at the noise level of nodes[-1].  lower_order_final None: on below 15
        steps.  Returns (z, x_inter, pred_x0_inter); the intermediates are None unless want_intermediates."""
        if lower_order_final is None:
            lower_order_final = _nodes_array(nodes).shape[0] - 1 < 15
        return self._sampler_call("dpmpp_sample", lib.rdm_dpmpp_sample, DpmppArgs, x_T, cond, uncond, alphas_cumprod, scale, log_every_t,
                                  want_intermediates, nodes=nodes, order=int(order), lower_order_final=int(bool(lower_order_final)))

    def op_dpmpp_step(self, x, eps, m_prev, cfg, scale, sqrt_a_s, sqrt_one_minus_a_s, c_x, c_0, c_1, x_out, x_dup=None, m_store=None,
                      pred_x0=None):
        """The DPM-Solver++ update kernel alone on caller-owned fp32 device tensors of x.numel() elements (eps: twice that under cfg,
        [cond | uncond]); m_prev / x_dup / m_store / pred_x0 may be None, m_store may be m_prev.  Writes into the given outputs."""
        n = self._step_sizes("op_dpmpp_step", x, eps, cfg, (m_prev, x_out, x_dup, m_store, pred_x0))
        self._check(lib.rdm_op_dpmpp_step(self._h, _ptr(x), _ptr(eps), _ptr(m_prev), n, int(bool(cfg)), float(scale), float(sqrt_a_s),
                                          float(sqrt_one_minus_a_s), float(c_x), float(c_0), float(c_1), _ptr(x_out), _ptr(x_dup),
                                          _ptr(m_store), _ptr(pred_x0)))

    def dpmpp_sde_sample(self, nodes, x_T, cond, uncond, alphas_cumprod, scale=1.0, order=2, lower_order_final=None, noise=None,
                         log_every_t=100, want_intermediates=False, seed=None, row0=0, shape=None):
        """SDE-DPM-Solver++(2M) over the node list of dpmpp_sample: rdm_dpmpp_sde_sample with `noise`, the [len(nodes) - 1, B, C, H, W] stack of
        the steps' z_j; with `seed` z_j is the library's own (seed, stream 1, step j, row0 + b), generated in
        the step kernel (`noise` must then be None), and x_T may be None -- the start is then drawn from stream 0 at the latent `shape`
        (C, H, W), for cond.shape[0] rows.  Returns (z, x_inter, pred_x0_inter); the intermediates are None unless want_intermediates."""
        if lower_order_final is None:
            lower_order_final = _nodes_array(nodes).shape[0] - 1 < 15
        if seed is None and (x_T is None or noise is None):
            raise RdmError("dpmpp_sde_sample: x_T and a noise stack are required without a seed")
        nz, noise, x_shape = _noise_source(self, "dpmpp_sde_sample", x_T, cond, noise, seed, row0, shape)
        return self._sampler_call("dpmpp_sde_sample", lib.rdm_dpmpp_sde_sample, DpmppArgs, x_T, cond, uncond, alphas_cumprod, scale, log_every_t,
                                  want_intermediates, nz=nz, noise=noise, x_shape=x_shape, nodes=nodes, order=int(order),
                                  lower_order_final=int(bool(lower_order_final)))

    def op_dpmpp_sde_step(self, x, eps, m_prev, noise, cfg, scale, sqrt_a_s, sqrt_one_minus_a_s, c_x, c_0, c_1, c_n, x_out, x_dup=None,
                          m_store=None, pred_x0=None, seed=None, row0=0, per_row=None, step=0):
        """The SDE-DPM-Solver++ update kernel alone on caller-owned fp32 device tensors of x.numel() elements (eps: twice that under cfg,
        [cond | uncond]) (rdm_op_dpmpp_sde_step); m_prev / x_dup / m_store / pred_x0 may be None, m_store may be m_prev.  With `seed` (and
        no noise) the noise of (seed, stream 1, step, row0 + b) for rows of per_row elements, drawn in the
        kernel.  Writes into the given outputs."""
        n = self._step_sizes("op_dpmpp_sde_step", x, eps, cfg, (m_prev, noise, x_out, x_dup, m_store, pred_x0))
        sc = [float(v) for v in (scale, sqrt_a_s, sqrt_one_minus_a_s, c_x, c_0, c_1, c_n)]
        outs = (_ptr(x_out), _ptr(x_dup), _ptr(m_store), _ptr(pred_x0))
        if seed is None and noise is None:
            raise RdmError("op_dpmpp_sde_step: a noise operand or a seed is required")
        nz = self._step_noise("op_dpmpp_sde_step", noise, n, seed, row0, per_row, step)
        self._check(lib.rdm_op_dpmpp_sde_step(self._h, _ptr(x), _ptr(eps), _ptr(m_prev), C.byref(nz), n, int(bool(cfg)), *sc, *outs))

    @staticmethod
    def unipc_coefficients(nodes, alphas_cumprod, j, order=2, variant="bh2", corrector=True, lower_order_final=True):
        return unipc_coefficients(nodes, alphas_cumprod, j, order, variant, corrector, lower_order_final)

    def unipc_sample(self, nodes, x_T, cond, uncond, alphas_cumprod, scale=1.0, order=2, variant="bh2", corrector=True,
                     lower_order_final=True, log_every_t=100, want_intermediates=False):
        """UniPC (Zhao et al. 2023; multistep data prediction, predictor order 1 | 2 | 3, the corrector adds one) over the strictly
        decreasing integer timesteps `nodes` (dpmpp_timesteps builds the two grids): len(nodes) - 1 UNet forwards, the result at the noise
        level of nodes[-1].  Returns (z, x_inter, pred_x0_inter): x_inter[j] the UNet input of node j + 1 (the last one is z),
        pred_x0_inter[j] = m_j; the intermediates are None unless want_intermediates."""
        return self._sampler_call("unipc_sample", lib.rdm_unipc_sample, UnipcArgs, x_T, cond, uncond, alphas_cumprod, scale, log_every_t,
                                  want_intermediates, nodes=nodes, order=int(order), variant=_unipc_variant("unipc_sample", variant),
                                  corrector=int(bool(corrector)), lower_order_final=int(bool(lower_order_final)))

    def op_unipc_step(self, u, eps, coefficients, cfg, scale, u_next, xc_prev=None, h1=None, h2=None, h3=None, xc_out=None, x_dup=None,
                      m_store=None, pred_x0=None):
        """The UniPC predict-and-correct kernel alone on caller-owned fp32 device tensors of u.numel() elements (eps: twice that under
        cfg, [cond | uncond]); `coefficients` the 13 float64 values of unipc_coefficients.  xc_prev / h1 / h2 / h3 as far as the orders
        reach; u_next may be u, xc_out may be xc_prev, m_store may be a history slot.  Writes into the given outputs."""
        co = np.ascontiguousarray(np.asarray(coefficients, dtype=np.float64).reshape(-1))
        if co.shape[0] != len(UNIPC_COEFFICIENTS):
            raise RdmError(f"op_unipc_step: coefficients must hold {len(UNIPC_COEFFICIENTS)} values")
        n = self._step_sizes("op_unipc_step", u, eps, cfg, (xc_prev, h1, h2, h3, xc_out, u_next, x_dup, m_store, pred_x0), name="u")
        self._check(lib.rdm_op_unipc_step(self._h, _ptr(u), _ptr(eps), _ptr(xc_prev), _ptr(h1), _ptr(h2), _ptr(h3), n, int(bool(cfg)),
                                          float(scale), co.ctypes.data_as(C.POINTER(C.c_double)), _ptr(xc_out), _ptr(u_next), _ptr(x_dup),
                                          _ptr(m_store), _ptr(pred_x0)))

    def ddpm_sample(self, timesteps, x_T, cond, noise=None, sched=None, clip_denoised=True, temperature=1.0, seed=None, row0=0, shape=None):
        """rdm_ddpm_sample on a noise stack [timesteps, B, C, H, W]; with `seed` (and no stack) the library's own
        noise, generated in the step kernel, and x_T may be None (drawn from stream 0 at the latent `shape` (C, H, W))."""
        if sched is None:
            raise RdmError("ddpm_sample: the schedule arrays are required")
        if seed is None and (noise is None or x_T is None):
            raise RdmError("ddpm_sample: x_T and a noise stack are required without a seed")
        nz, noise, x_shape = _noise_source(self, "ddpm_sample", x_T, cond, noise, seed, row0, shape)
        cond = self._dev(cond, torch.float32)
        x_arg = x_T = None if x_T is None else self._dev(x_T, torch.float32)
        if x_T is None:
            x_T = torch.empty(x_shape, device="meta", dtype=torch.float32)     # shapes only
        arrs = {k: np.ascontiguousarray(np.asarray(v, dtype=np.float32)) for k, v in sched.items()}
        fp = lambda k: arrs[k].ctypes.data_as(C.POINTER(C.c_float))
        self._check_sampler_shapes("ddpm_sample", x_T, cond, None, noise, int(timesteps))
        B, Cc, H, W = x_T.shape
        a = DdpmArgs(timesteps=timesteps, batch=B, k=cond.shape[1], channels=Cc, height=H, width=W,
                     clip_denoised=int(clip_denoised), temperature=temperature, T=arrs["posterior_mean_coef1"].shape[0],
                     sqrt_recip_alphas_cumprod=fp("sqrt_recip_alphas_cumprod"),
                     sqrt_recipm1_alphas_cumprod=fp("sqrt_recipm1_alphas_cumprod"),
                     posterior_mean_coef1=fp("posterior_mean_coef1"), posterior_mean_coef2=fp("posterior_mean_coef2"),
                     posterior_log_variance_clipped=fp("posterior_log_variance_clipped"))
        z = torch.empty(tuple(x_T.shape), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_ddpm_sample(self._h, C.byref(a), _ptr(x_arg), _ptr(cond), C.byref(nz), _ptr(z)))
        return z

    def vq_decode(self, z, force_not_quantize=False, return_indices=False):
        """decode_first_stage: latent f32 [b,embed_dim,h,w] -> image f32 [b,out_ch,f*h,f*w], f = 2^(levels-1); any h, w (the decoder is
        conv-only: rdm_vq_decode_hw), optionally the code indices int32 [b*h*w]."""
        z = self._dev(z, torch.float32)
        cfg = self._need("vq_decode", "vq")
        if z.ndim != 4 or z.shape[1] != cfg.embed_dim or min(z.shape) < 1:
            raise RdmError(f"vq_decode: latent must be [b,{cfg.embed_dim},h,w], got {tuple(z.shape)}")
        b, _, h, w = z.shape; f = 1 << (cfg.n_ch_mult - 1)
        img = torch.empty((b, cfg.out_ch, f * h, f * w), device=self.device, dtype=torch.float32)
        idx = torch.empty((b * h * w,), device=self.device, dtype=torch.int32) if return_indices else None
        self._check(lib.rdm_vq_decode_hw(self._h, _ptr(z), b, h, w, int(force_not_quantize), _ptr(img), _ptr(idx)))
        return (img, idx) if return_indices else img

    def vq_quantize(self, z, return_indices=False):
        """first_stage_model.quantize(z): z f32 [b,3,h,w] (any h, w) -> z_q (straight-through form), optionally the code indices."""
        z = self._dev(z, torch.float32)
        cfg = self._need("vq_quantize", "vq")
        if z.ndim != 4 or z.shape[1] != cfg.embed_dim or min(z.shape) < 1:
            raise RdmError(f"vq_quantize: latent must be [b,{cfg.embed_dim},h,w], got {tuple(z.shape)}")
        b, _, h, w = z.shape
        zq = torch.empty_like(z)
        idx = torch.empty((b * h * w,), device=self.device, dtype=torch.int32) if return_indices else None
        self._check(lib.rdm_vq_quantize_hw(self._h, _ptr(z), b, h, w, _ptr(zq), _ptr(idx)))
        return (zq, idx) if return_indices else zq

    def to_uint8(self, img):
        img = self._dev(img, torch.float32)
        b, c, h, w = img.shape
        out = torch.empty((b, h, w, c), device=self.device, dtype=torch.uint8)
        self._check(lib.rdm_to_uint8(self._h, _ptr(img), b, c, h, w, _ptr(out)))
        return out

    def clip_encode_text(self, tokens):
        tokens = self._dev(tokens, torch.int64)
        cfg = self._need("clip_encode_text", "clip")
        if tokens.ndim != 2 or tokens.shape[1] != cfg.context_length:
            raise RdmError(f"clip_encode_text: tokens must be [b,{cfg.context_length}], got {tuple(tokens.shape)}")
        self._check_ids("clip_encode_text", tokens, cfg.vocab_size, "tokens")      # (the embedding kernel indexes the table by the id as given)
        out = torch.empty((tokens.shape[0], self.clip_cfg.embed_dim), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_clip_encode_text(self._h, _ptr(tokens), tokens.shape[0], _ptr(out)))
        return out

    def clip_encode_image(self, image):
        image = self._dev(image, torch.float32)
        cfg = self._need("clip_encode_image", "clip")
        if image.ndim != 4 or tuple(image.shape[1:]) != (3, cfg.image_resolution, cfg.image_resolution):
            raise RdmError(f"clip_encode_image: image must be [b,3,{cfg.image_resolution},{cfg.image_resolution}] (already resized / normalised), got {tuple(image.shape)}")
        out = torch.empty((image.shape[0], self.clip_cfg.embed_dim), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_clip_encode_image(self._h, _ptr(image), image.shape[0], _ptr(out)))
        return out

    def clip_preprocess(self, image):
        """[b,3,h,w] in [-1,1] -> bicubic resize to the tower resolution + CLIP normalisation, f32 [b,3,R,R]."""
        image = self._dev(image, torch.float32)
        if image.ndim != 4 or image.shape[1] != 3:
            raise RdmError(f"clip_preprocess: image must be [b,3,h,w], got {tuple(image.shape)}")
        r = self._need("clip_preprocess", "clip").image_resolution
        out = torch.empty((image.shape[0], 3, r, r), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_clip_preprocess(self._h, _ptr(image), image.shape[0], image.shape[2], image.shape[3], _ptr(out)))
        return out

    def clip_encode_image_raw(self, image):
        """ClipImageRetriever.forward: preprocess fused into the image tower's patch gather."""
        image = self._dev(image, torch.float32)
        if image.ndim != 4 or image.shape[1] != 3:
            raise RdmError(f"clip_encode_image_raw: image must be [b,3,h,w], got {tuple(image.shape)}")
        self._need("clip_encode_image_raw", "clip")
        out = torch.empty((image.shape[0], self.clip_cfg.embed_dim), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_clip_encode_image_raw(self._h, _ptr(image), image.shape[0], image.shape[2], image.shape[3], _ptr(out)))
        return out

    # ---- retrieval
    def db_load(self, emb):
        """emb: numpy fp16/fp32 [n,dim] (host) or torch CUDA tensor (device)."""
        if isinstance(emb, torch.Tensor) and emb.is_cuda:
            emb = emb.contiguous()
            dt = {torch.float16: 0, torch.float32: 1}[emb.dtype]
            self._check(lib.rdm_db_load(self._h, _ptr(emb), emb.shape[0], emb.shape[1], dt, 1))
            self._db_dim = int(emb.shape[1])
        else:
            emb = np.ascontiguousarray(emb.numpy() if isinstance(emb, torch.Tensor) else emb)
            dt = {np.dtype(np.float16): 0, np.dtype(np.float32): 1}[emb.dtype]
            self._check(lib.rdm_db_load(self._h, emb.ctypes.data_as(_P), emb.shape[0], emb.shape[1], dt, 0))
            self._db_dim = int(emb.shape[1])

    def db_size(self):
        return int(lib.rdm_db_size(self._h))

    def knn(self, q, k, f64=False, allow=None, mask_of_query=None):
        """-> (idx int32 holding uint32 bits [b,k], score f32 [b,k]); f64=True: the fp64 scores the ranking was made on (shard merges).
        allow: int64 [n_masks, words] (or [words]) row masks on the device (row_mask), mask_of_query: one mask index per query (None:
        mask 0 for all) -- the exact top-k over the rows each query's mask allows (rdm_knn_filtered); a query with fewer than k allowed
        rows gets them followed by (NO_ROW, -inf).  allow=None: the unfiltered search."""
        q = self._dev(q, torch.float32)
        if q.ndim != 2:
            raise RdmError(f"knn: queries must be [b,dim], got {tuple(q.shape)}")
        allow, n_masks, ids = row_filter_args(allow, mask_of_query, q.shape[0], knn_mask_words(self.db_size()))
        idx = torch.empty((q.shape[0], k), device=self.device, dtype=torch.int32)   # uint32 bits
        sc = torch.empty((q.shape[0], k), device=self.device, dtype=torch.float64 if f64 else torch.float32)
        if allow is None:
            fn = lib.rdm_knn_f64 if f64 else lib.rdm_knn
            self._check(fn(self._h, _ptr(q), q.shape[0], k, _ptr(idx), _ptr(sc)))
        else:
            allow = self._dev(allow, torch.int64)
            fn = lib.rdm_knn_filtered_f64 if f64 else lib.rdm_knn_filtered
            self._check(fn(self._h, _ptr(q), q.shape[0], k, _ptr(allow), n_masks, None if ids is None else ids.ctypes.data_as(_P),
                           _ptr(idx), _ptr(sc)))
        return idx, sc

    def row_mask(self, rows_or_bool, invert=False):
        """-> int64 [words] on the device: the mask that allows the listed rows of the loaded database (rdm_op_row_mask).  Takes an index
        array or tensor (duplicates allowed), or a boolean array of length n; invert: the complement within [0, n)."""
        n = self.db_size()
        if n <= 0:
            raise RdmError("row_mask: no database loaded")
        r = rows_or_bool
        if isinstance(r, torch.Tensor):
            if r.dtype == torch.bool:
                if r.shape != (n,):
                    raise RdmError(f"row_mask: a boolean mask must have length {n}, got {tuple(r.shape)}")
                r = torch.nonzero(r.reshape(-1)).reshape(-1)
            r = r.reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        else:
            r = np.asarray(r)
            if r.dtype == np.bool_:
                if r.shape != (n,):
                    raise RdmError(f"row_mask: a boolean mask must have length {n}, got {r.shape}")
                r = np.flatnonzero(r)
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise RdmError(f"row_mask: row indices must be integers, got {r.dtype}")
            r = torch.from_numpy(np.ascontiguousarray(r.reshape(-1).astype(np.int64))).to(self.device)
        bits = torch.empty(knn_mask_words(n), device=self.device, dtype=torch.int64)
        self._check(lib.rdm_op_row_mask(self._h, _ptr(r) if r.numel() else None, r.numel(), n, int(bool(invert)), _ptr(bits)))
        return bits

    def row_mask_count(self, allow):
        """-> int64 numpy [n_masks]: allowed rows (below n) of each mask of allow int64 [n_masks, words] or [words]."""
        allow, n_masks, _ = row_filter_args(allow, None, 0, knn_mask_words(self.db_size()))
        if allow is None:
            raise RdmError("row_mask_count: allow is None")
        allow = self._dev(allow, torch.int64)
        out = np.zeros(n_masks, dtype=np.int64)
        self._check(lib.rdm_op_row_mask_count(self._h, _ptr(allow), n_masks, self.db_size(), out.ctypes.data_as(_P)))
        return out

    def knn_last_fallback(self):
        return int(lib.rdm_knn_last_fallback(self._h))

    def knn_stages(self, q, k, allow=None, mask_of_query=None):
        """Context.knn for ONE query group (b <= 64, or 128 <= b <= 512 on the bulk path) with every stage copied out (rdm_op_knn_stages):
        a dict with idx, score (the final answer), qn f32 / qh, ql fp16 [rows, dim] (rows b.. are padding), cand_s f32 / cand_i int32
        holding uint32 bits [rows, nlists, ksel], and per query the merge's flag, tau, tau_idx, theta BEFORE the exact fallback, plus the
        fields of knn_select.  allow / mask_of_query as in knn: the same read-out of the filtered search (rdm_op_knn_stages_filtered)."""
        q = self._dev(q, torch.float32)
        if q.ndim != 2:
            raise RdmError(f"knn_stages: queries must be [b,dim], got {tuple(q.shape)}")
        b, dim = q.shape
        n = self.db_size()
        allow, n_masks, ids = row_filter_args(allow, mask_of_query, b, knn_mask_words(n))
        form = knn_select(n, dim, b, k)
        rows = form["queries_per_launch"]
        ntiles = (n + 255) // 256
        cap = 8 * min(ntiles, torch.cuda.get_device_properties(self.device).multi_processor_count)
        dv = self.device
        t = {"idx": torch.empty((b, k), device=dv, dtype=torch.int32), "score": torch.empty((b, k), device=dv, dtype=torch.float32),
             "qn": torch.zeros((rows, dim), device=dv, dtype=torch.float32), "qh": torch.zeros((rows, dim), device=dv, dtype=torch.float16),
             "ql": torch.zeros((rows, dim), device=dv, dtype=torch.float16),
             "cand_s": torch.zeros(rows * cap * form["ksel"], device=dv, dtype=torch.float32),
             "cand_i": torch.zeros(rows * cap * form["ksel"], device=dv, dtype=torch.int32),
             "flag": torch.zeros(b, device=dv, dtype=torch.int32), "tau": torch.zeros(b, device=dv, dtype=torch.float64),
             "tau_idx": torch.zeros(b, device=dv, dtype=torch.int32), "theta": torch.zeros(b, device=dv, dtype=torch.float32)}
        st = KnnStages(rows_cap=rows, nlists_cap=cap)
        for name in ("qn", "qh", "ql", "cand_s", "cand_i", "flag", "tau", "tau_idx", "theta"):
            setattr(st, name, t[name].data_ptr())
        if allow is None:
            self._check(lib.rdm_op_knn_stages(self._h, _ptr(q), b, k, _ptr(t["idx"]), _ptr(t["score"]), C.byref(st)))
        else:
            allow = self._dev(allow, torch.int64)
            self._check(lib.rdm_op_knn_stages_filtered(self._h, _ptr(q), b, k, _ptr(allow), n_masks,
                                                       None if ids is None else ids.ctypes.data_as(_P), _ptr(t["idx"]), _ptr(t["score"]), C.byref(st)))
        used = st.rows * st.nlists * st.form.ksel
        for name in ("qn", "qh", "ql"):
            t[name] = t[name][:st.rows]
        for name in ("cand_s", "cand_i"):
            t[name] = t[name][:used].reshape(st.rows, st.nlists, st.form.ksel)
        t.update(form)
        return t

    def db_rows(self, row0, rows):
        """-> fp16 [rows, dim]: the normalised database rows [row0, row0 + rows) the search scores (rdm_db_rows)."""
        dim = self._db_dim
        out = torch.empty((rows, dim), device=self.device, dtype=torch.float16)
        self._check(lib.rdm_db_rows(self._h, int(row0), int(rows), _ptr(out)))
        return out

    def db_gather(self, idx, dim):
        idx = idx.contiguous()
        out = torch.empty((idx.numel(), dim), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_db_gather(self._h, _ptr(idx), idx.numel(), _ptr(out)))
        return out.reshape(tuple(idx.shape) + (dim,))

    # ---- measurement
    def prof_enable(self, kinds=(0, 1)):
        """kinds: iterable of PROF_* kernel classes to bracket with HIP events (False / () = off; True = conv3x3 + linear)."""
        if kinds is True:
            kinds = (PROF_CONV3X3, PROF_LINEAR)
        mask = 0
        for k in (kinds or ()):
            mask |= 1 << int(k)
        self._check(lib.rdm_prof_enable(self._h, mask))

    def set_deterministic(self, on: bool = True):
        """Batch-invariant execution (include/rdm_hip.h rdm_set_deterministic): bitwise the same row whatever batch / rank count."""
        self._check(lib.rdm_set_deterministic(self._h, int(bool(on))))

    @property
    def deterministic(self) -> bool:
        return lib.rdm_get_deterministic(self._h) == 1

    def set_neighbour_bias(self, bias):
        """The additive per-(sample, neighbour) term on the UNet's cross-attention scores (include/rdm_hip.h rdm_set_neighbour_bias):
        bias [B, k] (0 = unbiased, log w = counts w times, -inf = absent), in force for every UNet forward and sampler call of B
        conditional samples x k neighbours until replaced or cleared (None).  Refused: NaN, +inf, a row without a finite entry."""
        if bias is None:
            self._check(lib.rdm_set_neighbour_bias(self._h, None, 0, 0))
            self._nn_bias = None
            return
        b = torch.as_tensor(bias).detach().to("cpu", torch.float32).contiguous()
        if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1:
            raise RdmError(f"set_neighbour_bias: the bias must be [B, k], got {tuple(b.shape)}")
        self._check(lib.rdm_set_neighbour_bias(self._h, C.c_void_p(b.data_ptr()), b.shape[0], b.shape[1]))
        self._nn_bias = b.clone()            # (the host copy: what neighbour_bias_doubled restores)

    def get_neighbour_bias(self):
        """(rows, k) of the bias in force, or None."""
        r, k = C.c_int(0), C.c_int(0)
        return (r.value, k.value) if lib.rdm_get_neighbour_bias(self._h, C.byref(r), C.byref(k)) == 1 else None

    @contextlib.contextmanager
    def neighbour_bias_doubled(self, uncond_first=False):
        """For a per-step path's guided forward, which runs unet_forward on the doubled batch [c | uc] ([uc | c] with uncond_first): the
        bias in force, [B, k], becomes [bias | zeros] ([zeros | bias]) for the block -- the unconditional half is never biased -- and is put
        back afterwards.  Without a bias in force nothing happens."""
        b = getattr(self, "_nn_bias", None)
        if b is None:
            yield
            return
        z = torch.zeros_like(b)
        self.set_neighbour_bias(torch.cat([z, b] if uncond_first else [b, z]))
        try:
            yield
        finally:
            self.set_neighbour_bias(b)

    @contextlib.contextmanager
    def neighbour_bias(self, bias):
        """`with ctx.neighbour_bias(bias): ...`: set for the block (None: nothing is set), cleared on the way out whatever happens."""
        if bias is None:
            yield
            return
        self.set_neighbour_bias(bias)
        try:
            yield
        finally:
            self.set_neighbour_bias(None)

    # ---- RCCL through the C ABI (include/rdm_hip.h "multi-GPU"); the package's own multi-GPU path uses torch.distributed
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._check(lib.rdm_comm_unique_id(self._h, buf))
        return buf.raw

    def new_comm_context(self):
        """A sibling context on the same device whose ONLY job is to own the RCCL communicator (parallel.attach_library_comm): its stream is a
        fresh non-blocking side stream, so a rendezvous or probe collective that never completes can block nothing but that stream, and a
        context that failed its hand-shake is simply abandoned (advisor, round 5: a late helper thread must not share the product context,
        which is not thread-safe, nor enqueue on the product's stream)."""
        c = Context(self.device.index)
        c._side_stream = torch.cuda.Stream(self.device)
        c._check(lib.rdm_set_stream(c._h, C.c_void_p(c._side_stream.cuda_stream)))
        return c

    def comm_init(self, uid: bytes, rank: int, world: int):
        if len(uid) != 128:
            raise RdmError(f"comm_init: the unique id is 128 bytes, got {len(uid)}")
        self._check(lib.rdm_comm_init(self._h, C.create_string_buffer(uid, 128), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_all_gather(self, local: torch.Tensor, world: int) -> torch.Tensor:
        local = local.contiguous()
        out = torch.empty((world,) + tuple(local.shape), device=self.device, dtype=local.dtype)
        self._check(lib.rdm_comm_all_gather(self._h, _ptr(local), _ptr(out), local.numel() * local.element_size()))
        return out

    def comm_all_reduce(self, buf: torch.Tensor, average=True):
        """In-place sum (mean) over the ranks of an fp32 device tensor through the context's RCCL communicator."""
        if buf.dtype != torch.float32 or not buf.is_contiguous():
            raise RdmError("comm_all_reduce: contiguous float32 tensor required")
        self._check(lib.rdm_comm_all_reduce_f32(self._h, _ptr(buf), buf.numel(), int(bool(average))))
        return buf

    def comm_destroy(self):
        self._check(lib.rdm_comm_destroy(self._h))
        self.comm_world = 0

    def prof_reset(self):
        self._check(lib.rdm_prof_reset(self._h))

    def debug_tap(self, buf, block, sub=0):
        """The next forwards copy one intermediate activation (block `block`, stage `sub`: include/rdm_hip.h) into `buf`; buf None: off.
        UNet blocks (0 ..), first-stage decoder layers (1000 ..) and encoder layers (1500 ..) show bf16 tensors; the CLIP text tower (block 2000) and image tower
        (block 3000) show each stage in the type it is stored in, fp32 or bf16 (the table in rdm_hip.h): `buf` is a device tensor of
        that type, and at most its numel * element_size bytes are written."""
        self._tap_keepalive = buf
        self._check(lib.rdm_debug_tap(self._h, _ptr(buf) if buf is not None else None, 0 if buf is None else buf.numel() * buf.element_size(), int(block), int(sub)))

    def debug_guidance_prefix(self, through_attn1=1):
        """Where the shared guidance prefix of a guided forward ends (rdm_debug_guidance_prefix): 1 (default) at the first transformer's
        attn1.to_out, 0 in front of that transformer.  Both give the same bits; the hook exists to compare them in one process."""
        self._check(lib.rdm_debug_guidance_prefix(self._h, int(through_attn1)))

    def calib_probe(self, mfma_ms=800.0, stream_bytes=1 << 30, stream_reps=6):
        """Box calibration (rdm_calib_probe): (sustained dense-bf16 MFMA TFLOP/s on random operands, HBM copy GB/s read + write)."""
        buf = torch.empty(max(1 << 20, 2 * stream_bytes), device=self.device, dtype=torch.uint8)
        tf, gb = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.rdm_calib_probe(self._h, _ptr(buf), buf.numel(), float(mfma_ms), int(stream_bytes), int(stream_reps), C.byref(tf), C.byref(gb)))
        del buf
        return float(tf.value), float(gb.value)

    def prof_dump(self, path):
        """One CSV row per recorded launch (kind, role tag, shape, ms, work): tools/op_trace.py."""
        self._check(lib.rdm_prof_dump(self._h, os.fsencode(path)))

    def prof_collect(self, kind):
        n, ms, fl = C.c_longlong(0), C.c_double(0), C.c_double(0)
        self._check(lib.rdm_prof_collect(self._h, kind, C.byref(n), C.byref(ms), C.byref(fl)))
        return int(n.value), float(ms.value), float(fl.value)

    # ---- operator-level (parity tests)
    def op_linear(self, a, w, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out_f32=False):
        M, K = a.shape; N = w.shape[0]
        No = N // 2 if act == ACT_GEGLU else N
        ob = None if out_f32 else torch.empty((M, No), device=self.device, dtype=torch.bfloat16)
        of = torch.empty((M, No), device=self.device, dtype=torch.float32) if out_f32 else None
        self._check(lib.rdm_op_linear(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(ob), _ptr(of), M, N, K,
                                      act, float(alpha)))
        return of if out_f32 else ob

    def op_linear_rowvec(self, a, w, bias, rowvec, rows_per_group, residual=None):
        """a w^T + bias + rowvec[row // rows_per_group] (+ residual): rowvec f32 [groups, N]."""
        M, K = a.shape; N = w.shape[0]
        assert rowvec.dtype == torch.float32 and rowvec.shape == ((M + rows_per_group - 1) // rows_per_group, N) and rowvec.is_contiguous()
        out = torch.empty((M, N), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_linear_rowvec(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(rowvec), int(rows_per_group), _ptr(residual), _ptr(out), M, N, K))
        return out

    def op_linear_ln(self, x, w, bias, gamma, beta, act=ACT_NONE, eps=1e-5):
        """act(LayerNorm(x) w^T + bias) with the LayerNorm folded into the GEMM (raises RdmError for shapes the folded kernel does not take)."""
        M, K = x.shape; N = w.shape[0]
        out = torch.empty((M, N // 2 if act == ACT_GEGLU else N), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_linear_ln(self._h, _ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(out), M, N, K, act, float(eps)))
        return out

    def op_conv3x3(self, x0, w, bias, x1=None, rowvec=None, residual=None, stride=1, ups=0):
        B, Hin, Win, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[3]
        N = w.shape[0]
        Ho = Hin * 2 if ups else (Hin // 2 if stride == 2 else Hin)
        Wo = Win * 2 if ups else (Win // 2 if stride == 2 else Win)
        out = torch.empty((B, Ho, Wo, N), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_conv3x3(self._h, _ptr(x0), _ptr(x1), C0, C1, _ptr(w), _ptr(bias), _ptr(rowvec),
                                       0 if rowvec is None else rowvec.shape[1], _ptr(residual), _ptr(out), B, Hin, Win, N,
                                       stride, ups))
        return out

    def op_conv3x3_down(self, x, w, bias):
        """The first-stage encoder's Downsample conv (rdm_op_conv3x3_down): F.pad(x, (0, 1, 0, 1)) + a 3x3 conv of stride 2 without padding.
        x bf16 [B, Hin, Win, C], w bf16 [N, 3, 3, C], bias f32 [N] or None -> bf16 [B, Hin / 2, Win / 2, N]; odd Hin or Win raise RdmError."""
        B, Hin, Win, Cc = x.shape
        N = w.shape[0]
        out = torch.empty((B, Hin // 2, Win // 2, N), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_conv3x3_down(self._h, _ptr(x), Cc, _ptr(w), _ptr(bias), _ptr(out), B, Hin, Win, N))
        return out

    def op_rarm_sampler(self, logits, uniforms, guidance_scale=1.0, temperature=1.0, top_k=None, top_p=None, return_kept=False):
        """The sampler kernel alone: logits f32 [(2 if guided else 1) * b, vocab] (conditional rows first), uniforms f32 [b] -> int64 [b].
        top_p in (0, 1]: nucleus filter after top-k; None or 1.0: none.  return_kept: -> (tokens, int32 [b] tokens each row kept)."""
        top_p = check_top_p("op_rarm_sampler", top_p)
        logits = self._dev(logits, torch.float32); uniforms = self._dev(uniforms, torch.float32)
        b = uniforms.shape[0]
        cfg = guidance_scale > 1.0
        if logits.ndim != 2 or logits.shape[0] != (2 * b if cfg else b):
            raise RdmError(f"op_rarm_sampler: logits must be [{2 * b if cfg else b}, vocab], got {tuple(logits.shape)}")
        out = torch.empty((b,), device=self.device, dtype=torch.int64)
        k = int(top_k) if top_k is not None else 0
        if top_p is None and not return_kept:
            self._check(lib.rdm_op_rarm_sampler(self._h, _ptr(logits), b, logits.shape[1], int(cfg), float(guidance_scale), float(temperature),
                                                k, _ptr(uniforms), _ptr(out)))
            return out
        kept = torch.empty((b,), device=self.device, dtype=torch.int32) if return_kept else None
        self._check(lib.rdm_op_rarm_sampler_top_p(self._h, _ptr(logits), b, logits.shape[1], int(cfg), float(guidance_scale), float(temperature),
                                                  k, 1.0 if top_p is None else top_p, _ptr(uniforms), _ptr(out), _ptr(kept)))
        return (out, kept) if return_kept else out

    # ---- backward building blocks (include/rdm_hip.h "backward"; composed in rdm_amd/training.py)
    def op_conv3x3_dgrad(self, dy, w):
        B, H, W, N = dy.shape
        Cc = w.shape[3]
        dx = torch.empty((B, H, W, Cc), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_conv3x3_dgrad(self._h, _ptr(dy), _ptr(w), _ptr(dx), B, H, W, Cc, N))
        return dx

    def op_conv3x3_wgrad(self, x, dy):
        B, H, W, Cc = x.shape
        N = dy.shape[3]
        dw = torch.empty((N, 3, 3, Cc), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_conv3x3_wgrad(self._h, _ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cc, N))
        return dw

    def op_groupnorm_bwd(self, x, dy, gamma, beta, eps, silu, residual=None):
        """-> dx (+ residual when given: the skip path's gradient joins inside the kernel), dgamma, dbeta."""
        B, HW, Cc = x.shape
        dx = torch.empty_like(x); dg = torch.empty((Cc,), device=self.device, dtype=torch.float32); db = torch.empty_like(dg)
        assert residual is None or (residual.is_contiguous() and residual.numel() == x.numel())
        self._check(lib.rdm_op_groupnorm_bwd_add(self._h, _ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), B, HW, Cc, float(eps), int(silu), _ptr(residual),
                                                 _ptr(dx), _ptr(dg), _ptr(db)))
        return dx, dg, db

    def op_layernorm_bwd(self, x, dy, gamma, eps=1e-5, residual=None):
        M, Cc = x.shape
        dx = torch.empty_like(x); dg = torch.empty((Cc,), device=self.device, dtype=torch.float32); db = torch.empty_like(dg)
        assert residual is None or (residual.is_contiguous() and residual.numel() == x.numel())
        self._check(lib.rdm_op_layernorm_bwd_add(self._h, _ptr(x), _ptr(dy), _ptr(gamma), M, Cc, float(eps), _ptr(residual), _ptr(dx), _ptr(dg), _ptr(db)))
        return dx, dg, db

    def op_colsum(self, x):
        M, N = x.shape
        out = torch.empty((N,), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_colsum(self._h, _ptr(x), _ptr(out), M, N))
        return out

    def op_transpose(self, x):
        r, c_ = x.shape
        y = torch.empty((c_, r), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_transpose(self._h, _ptr(x), _ptr(y), r, c_))
        return y

    def op_add(self, a, b):
        out = torch.empty_like(a)
        self._check(lib.rdm_op_add(self._h, _ptr(a), _ptr(b), _ptr(out), a.numel()))
        return out

    def op_linear_wgrad(self, dy, a):
        """dy bf16 [M, N], a bf16 [M, K] -> dy^T a fp32 [N, K] (the weight gradient of y = a w^T)."""
        M, N = dy.shape; K = a.shape[1]
        dw = torch.empty((N, K), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_linear_wgrad(self._h, _ptr(dy), _ptr(a), _ptr(dw), M, N, K))
        return dw

    @staticmethod
    def _ptr_array(ts, optional=False):
        arr = (C.c_void_p * len(ts))()
        for i, t in enumerate(ts):
            if t is None:
                assert optional
                arr[i] = None
            else:
                assert t.is_contiguous(), "tensor must be contiguous"
                arr[i] = t.data_ptr()
        return arr

    def op_adamw_multi(self, ps, gs, ms, vs, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, p_bf16s=None):
        """op_adamw over lists of fp32 tensors (48 tensors per launch); p_bf16s: list with None where a tensor has no bf16 working copy."""
        n = len(ps)
        assert n == len(gs) == len(ms) == len(vs) and all(g.numel() == p.numel() and g.dtype == torch.float32 for p, g in zip(ps, gs))
        numel = (C.c_longlong * n)(*[p.numel() for p in ps])
        self._check(lib.rdm_op_adamw_multi(self._h, n, self._ptr_array(ps), self._ptr_array(gs), self._ptr_array(ms), self._ptr_array(vs),
                                           self._ptr_array(p_bf16s, True) if p_bf16s is not None else None, numel, float(lr), float(betas[0]),
                                           float(betas[1]), float(eps), float(weight_decay), int(step)))

    def op_ema_multi(self, shadows, ps, one_minus_decay):
        n = len(ps)
        numel = (C.c_longlong * n)(*[p.numel() for p in ps])
        self._check(lib.rdm_op_ema_multi(self._h, n, self._ptr_array(shadows), self._ptr_array(ps), numel, float(one_minus_decay)))

    def op_ema(self, shadow, p, one_minus_decay):
        self._check(lib.rdm_op_ema(self._h, _ptr(shadow), _ptr(p), p.numel(), float(one_minus_decay)))

    def op_silu(self, x, dy=None):
        """x fp32: -> silu(x) bf16, or with dy (fp32) the gradient dy * silu'(x) fp32."""
        out = torch.empty(x.shape, device=self.device, dtype=torch.bfloat16 if dy is None else torch.float32)
        self._check(lib.rdm_op_silu(self._h, _ptr(x), _ptr(dy) if dy is not None else None, _ptr(out), x.numel()))
        return out

    # ---- training-step glue (include/rdm_hip.h: rdm_op_q_sample ...)
    def op_q_sample(self, x0, noise, sqrt_ac, sqrt_1mac, want_nchw=True, cpad=0):
        """x_t = sqrt_ac[b] x0 + sqrt_1mac[b] noise: -> (f32 NCHW or None, bf16 NHWC [B,H,W,cpad] or None)."""
        B, Cc, H, W = x0.shape
        out = torch.empty_like(x0) if want_nchw else None
        onh = torch.empty((B, H, W, cpad), device=self.device, dtype=torch.bfloat16) if cpad else None
        self._check(lib.rdm_op_q_sample(self._h, _ptr(x0), _ptr(noise), _ptr(sqrt_ac), _ptr(sqrt_1mac), _ptr(out), _ptr(onh), B, Cc, H, W, cpad))
        return out, onh

    def op_mse_loss(self, eps_nhwc, target, coef=None, C_=None):
        """eps bf16 [B,H,W,ldc], target f32 [B,C,H,W] -> (se f32 [B], deps bf16 [B,H,W,ldc] = coef[b] (eps - target), or None without coef)."""
        B, H, W, ldc = eps_nhwc.shape
        Cc = target.shape[1] if C_ is None else C_
        se = torch.empty((B,), device=self.device, dtype=torch.float32)
        deps = torch.empty_like(eps_nhwc) if coef is not None else None
        self._check(lib.rdm_op_mse_loss(self._h, _ptr(eps_nhwc), _ptr(target), _ptr(coef), _ptr(se), _ptr(deps), B, Cc, H, W, ldc))
        return se, deps

    def op_where_rows(self, mask, a, x):
        """out[b] = a[b] if mask[b] else x[b]; mask uint8 / bool [B], a / x f32 [B, ...]."""
        out = torch.empty_like(x)
        m8 = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(lib.rdm_op_where_rows(self._h, _ptr(m8), _ptr(a), _ptr(x), _ptr(out), x.shape[0], x[0].numel()))
        return out

    def op_timestep_embedding(self, t, dim, ld=None):
        ld = dim if ld is None else ld
        out = torch.empty((t.shape[0], ld), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_timestep_embedding(self._h, _ptr(t), _ptr(out), t.shape[0], dim, ld))
        return out

    def op_colsum_samples(self, x):
        """x bf16 [B, HW, N] -> bf16 [B, N]."""
        B, HW, N = x.shape
        out = torch.empty((B, N), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_colsum_samples(self._h, _ptr(x), _ptr(out), B, HW, N))
        return out

    def op_expand2(self, x, mode):
        """x bf16 [B,H,W,C] -> [B,2H,2W,C]: mode 0 zero insertion, mode 1 nearest-neighbour copy."""
        B, H, W, Cc = x.shape
        out = torch.empty((B, 2 * H, 2 * W, Cc), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_expand2(self._h, _ptr(x), _ptr(out), B, H, W, Cc, mode))
        return out

    def op_sumpool2(self, x):
        B, H2, W2, Cc = x.shape
        out = torch.empty((B, H2 // 2, W2 // 2, Cc), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_sumpool2(self._h, _ptr(x), _ptr(out), B, H2 // 2, W2 // 2, Cc))
        return out

    def op_adamw(self, p, g, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, p_bf16=None):
        """In-place AdamW step on fp32 tensors p / m / v with gradient g; p_bf16 (same shape, bf16) receives the rounded new parameters."""
        self._check(lib.rdm_op_adamw(self._h, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16) if p_bf16 is not None else None, p.numel(),
                                     float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step)))

    def op_attention_bwd(self, q, k, v, o, dout, heads):
        """fused attention backward (d_head 32): q / o / dout bf16 [B, n, C], k / v [B, m, C] -> dq, dk, dv."""
        B, n, _ = q.shape; m = k.shape[1]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        self._check(lib.rdm_op_attention_bwd(self._h, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(dout), B, n, m, heads, _ptr(dq), _ptr(dk), _ptr(dv)))
        return dq, dk, dv

    def op_bmm(self, a, w, alpha=1.0, out_f32=False):
        """a bf16 [Z, M, K], w bf16 [Z, N, K] -> alpha * a w^T [Z, M, N] (bf16, or fp32 with out_f32)."""
        Z, M, K = a.shape; N = w.shape[1]
        out = torch.empty((Z, M, N), device=self.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
        self._check(lib.rdm_op_bmm(self._h, _ptr(a), _ptr(w), None if out_f32 else _ptr(out), _ptr(out) if out_f32 else None, Z, M, N, K, float(alpha)))
        return out

    def op_heads(self, x, H, D, mode, n=None):
        """mode 0 / 1: x bf16 [B, n, >= H D] -> per-head [B H, n, 64] / transposed [B H, 64, n]; mode 2: [B H, n, 64] -> [B, n, H D]."""
        if mode == 2:
            BH, n_, _ = x.shape; B = BH // H
            out = torch.empty((B, n_, H * D), device=self.device, dtype=torch.bfloat16)
            self._check(lib.rdm_op_heads(self._h, _ptr(x), _ptr(out), B, n_, H, D, H * D, 2))
            return out
        B, n_, ldx = x.shape
        out = torch.empty((B * H, n_, 64) if mode == 0 else (B * H, 64, n_), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_heads(self._h, _ptr(x), _ptr(out), B, n_, H, D, ldx, mode))
        return out

    def op_transpose_batched(self, x):
        Z, r, c_ = x.shape
        y = torch.empty((Z, c_, r), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_transpose_batched(self._h, _ptr(x), _ptr(y), Z, r, c_))
        return y

    def op_softmax(self, s, n_valid=0):
        p = torch.empty(s.shape, device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_softmax(self._h, _ptr(s), _ptr(p), s.numel() // s.shape[-1], s.shape[-1], int(n_valid)))
        return p

    def op_softmax_bwd(self, p, dp):
        ds = torch.empty_like(p)
        self._check(lib.rdm_op_softmax_bwd(self._h, _ptr(p), _ptr(dp), _ptr(ds), p.numel() // p.shape[-1], p.shape[-1]))
        return ds

    def op_geglu(self, pre, dh=None):
        """pre bf16 [M, 2F] = [x | gate] (unpermuted).  dh None -> x * gelu(gate) [M, F]; else the gradient [dx | dgate] [M, 2F]."""
        M, F2 = pre.shape
        out = torch.empty((M, F2 // 2) if dh is None else (M, F2), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_geglu(self._h, _ptr(pre), _ptr(dh) if dh is not None else None, _ptr(out), M, F2 // 2))
        return out

    def op_groupnorm(self, x0, gamma, beta, eps, silu, x1=None):
        B, HW, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[2]
        out = torch.empty((B, HW, C0 + C1), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_groupnorm(self._h, _ptr(x0), _ptr(x1), C0, C1, B, HW, _ptr(gamma), _ptr(beta), float(eps),
                                         int(silu), _ptr(out)))
        return out

    def op_layernorm(self, x, gamma, beta, eps=1e-5):
        M, Cc = x.shape
        out = torch.empty((M, Cc), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_layernorm(self._h, _ptr(x), int(x.dtype == torch.float32), _ptr(gamma), _ptr(beta), M, Cc,
                                         float(eps), _ptr(out)))
        return out

    def op_layernorm_f32(self, x, gamma, beta, eps=1e-5):
        """LayerNorm of fp32 rows to fp32 (the image tower's ln_pre)."""
        assert x.dtype == torch.float32
        M, Cc = x.shape
        out = torch.empty((M, Cc), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_layernorm_f32(self._h, _ptr(x), _ptr(gamma), _ptr(beta), M, Cc, float(eps), _ptr(out)))
        return out

    def op_linear_res_f32(self, a, w, bias=None, res=None, act=ACT_NONE, inplace=False):
        """act(a w^T + bias) + res -> fp32 through the tiled GEMM (the CLIP towers' residual adds).  res fp32 [M, N] or None;
        inplace: the output is written over `res` (the executors' form), which is returned; else into a fresh tensor."""
        M, K = a.shape; N = w.shape[0]
        assert res is None or (res.dtype == torch.float32 and tuple(res.shape) == (M, N))
        assert not inplace or res is not None
        out = res if inplace else torch.empty((M, N), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_linear_res_f32(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(res), _ptr(out), M, N, K, int(act)))
        return out

    def op_self_attention(self, qk, vt, heads):
        B, n, C2 = qk.shape
        out = torch.empty((B, n, C2 // 2), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_self_attention(self._h, _ptr(qk), _ptr(vt), B, n, heads, _ptr(out)))
        return out

    def op_self_attention_qkv(self, qkv, heads):
        """qkv bf16 [B, n, 3C] = [q | k | v] (one fused projection), n % 64 == 0 -> [B, n, C]."""
        B, n, C3 = qkv.shape
        out = torch.empty((B, n, C3 // 3), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_self_attention_qkv(self._h, _ptr(qkv), B, n, heads, _ptr(out)))
        return out

    def op_head_conv(self, x, w, bias, gn=None):
        """GroupNorm(32) + SiLU (gn = (gamma, beta, eps); None: no norm) + 3x3 conv to few channels: x bf16 [B, H, W, C], w fp32 [Cout, C, 3, 3]
        -> fp32 [B, Cout, H, W]."""
        B, H, W, Cc = x.shape
        Cout = w.shape[0]
        out = torch.empty((B, Cout, H, W), device=self.device, dtype=torch.float32)
        g, b_, eps = gn if gn is not None else (None, None, 0.0)
        opt = lambda t: _ptr(t) if t is not None else None
        self._check(lib.rdm_op_head_conv(self._h, _ptr(x), opt(g), opt(b_), float(eps), _ptr(w), opt(bias), B, H, W, Cc, Cout, _ptr(out)))
        return out

    def op_conv_in(self, x, w, bias):
        """the stem conv (conv_in_kernel): x fp32 [B, Cin, H, W] (Cin <= 4), w fp32 [Cout, Cin, 3, 3], bias fp32 [Cout] -> bf16 [B, H, W, Cout]."""
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        out = torch.empty((B, H, W, Cout), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_conv_in(self._h, _ptr(x), _ptr(w), _ptr(bias), B, Cin, H, W, Cout, _ptr(out)))
        return out

    def op_conv_out(self, x, w, bias):
        """the VALU head conv (conv_out_kernel, the models' fallback where op_head_conv refuses a shape): x bf16 [B, H, W, Cin], w fp32
        [Cout, Cin, 3, 3] (Cout <= 4), bias fp32 [Cout] -> fp32 [B, Cout, H, W]."""
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        out = torch.empty((B, Cout, H, W), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_conv_out(self._h, _ptr(x), _ptr(w), _ptr(bias), B, H, W, Cin, Cout, _ptr(out)))
        return out

    def _key_bias(self, what, key_bias, B, m):
        kb = self._dev(key_bias, torch.float32).contiguous()
        if tuple(kb.shape) != (B, m):
            raise RdmError(f"{what}: key_bias must be [{B}, {m}], got {tuple(kb.shape)}")
        return kb

    def op_xattn_fused(self, x, G, U, bias, res, ncols, group, ln=None, key_bias=None):
        """out = softmax_groups(x G^T) U^T + bias + res per sample: x / res bf16 [B, n, C], G bf16 [B, NP, C], U bf16 [B, C, NP].
        ln = (gamma, beta, eps): scores on LayerNorm(x), residual = x (res must be None).  key_bias fp32 [B, group]: the neighbour
        bias, added to the score columns h * group + j before the softmax (-inf: neighbour j is absent)."""
        B, n, Cc = x.shape
        NP = G.shape[1]
        out = torch.empty((B, n, Cc), device=self.device, dtype=torch.bfloat16)
        g, b_, eps = ln if ln is not None else (None, None, 0.0)
        opt = lambda t: _ptr(t) if t is not None else None
        if key_bias is not None:
            kb = self._key_bias("op_xattn_fused", key_bias, B, group)
            self._check(lib.rdm_op_xattn_fused_biased(self._h, _ptr(x), opt(g), opt(b_), float(eps), _ptr(G), _ptr(U), opt(bias), opt(res),
                                                      B, n, Cc, NP, ncols, group, _ptr(out), None, None, None, _ptr(kb)))
            return out
        self._check(lib.rdm_op_xattn_fused(self._h, _ptr(x), opt(g), opt(b_), float(eps), _ptr(G), _ptr(U), opt(bias), opt(res),
                                           B, n, Cc, NP, ncols, group, _ptr(out)))
        return out

    def op_xattn_fused_ln3(self, x, G, U, bias, ncols, group, ln, ln3, key_bias=None):
        """IN PLACE x <- softmax_groups(LayerNorm(x; ln) G^T) U^T + bias + x, and -> LayerNorm(new x; ln3) (bf16).  ln / ln3 = (gamma, beta[, eps]).
        key_bias: as in op_xattn_fused."""
        B, n, Cc = x.shape
        assert x.is_contiguous() and x.dtype == torch.bfloat16
        out3 = torch.empty_like(x)
        opt = lambda t: _ptr(t) if t is not None else None
        if key_bias is not None:
            kb = self._key_bias("op_xattn_fused_ln3", key_bias, B, group)
            self._check(lib.rdm_op_xattn_fused_biased(self._h, _ptr(x), _ptr(ln[0]), _ptr(ln[1]), float(ln[2] if len(ln) > 2 else 1e-5), _ptr(G), _ptr(U),
                                                      opt(bias), None, B, n, Cc, G.shape[1], ncols, group, None, _ptr(ln3[0]), _ptr(ln3[1]), _ptr(out3), _ptr(kb)))
            return out3
        self._check(lib.rdm_op_xattn_fused_ln3(self._h, _ptr(x), _ptr(ln[0]), _ptr(ln[1]), float(ln[2] if len(ln) > 2 else 1e-5), _ptr(G), _ptr(U), opt(bias),
                                               B, n, Cc, G.shape[1], ncols, group, _ptr(ln3[0]), _ptr(ln3[1]), _ptr(out3)))
        return out3

    def op_small_attention_bwd(self, q, k, v, dout, heads, scale):
        """Gradient of op_small_attention at d_head 32 with 1..32 keys (the UNet's cross-attention): -> dq, dk, dv (bf16)."""
        B, nq, Cc = q.shape
        m = k.shape[1]
        assert k.stride(-2) == v.stride(-2) and q.is_contiguous() and dout.is_contiguous()
        dq = torch.empty((B, nq, heads * 32), device=self.device, dtype=torch.bfloat16)
        dk = torch.empty((B, m, heads * 32), device=self.device, dtype=torch.bfloat16); dv = torch.empty_like(dk)
        self._check(lib.rdm_op_small_attention_bwd(self._h, _ptr(q), Cc, _ptr(k), _ptr(v), k.shape[2], _ptr(dout), dout.shape[2], B, nq, m, heads, float(scale),
                                                   _ptr(dq), _ptr(dk), _ptr(dv)))
        return dq, dk, dv

    def op_causal_attention_d64(self, qkv, heads, scale, kcache=None, vcache=None):
        """Causal self-attention at d_head 64 over all positions: qkv bf16 [B,n,3*heads*64] (q | k | v) -> bf16 [B,n,heads*64].
        kcache / vcache bf16 [B,heads,L,64]: rows 0..n-1 receive the K / V columns of qkv."""
        B, n, C3 = qkv.shape
        assert qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and C3 == 3 * heads * 64
        if n < 1 or n > 1024:
            raise RdmError(f"op_causal_attention_d64: 1 <= n <= 1024 required, got {n}")
        if (kcache is None) != (vcache is None):
            raise RdmError("op_causal_attention_d64: kcache and vcache come together")
        L = 0
        if kcache is not None:
            L = kcache.shape[2]
            if tuple(kcache.shape) != (B, heads, L, 64) or kcache.shape != vcache.shape or L < n:
                raise RdmError(f"op_causal_attention_d64: caches must be [{B},{heads},L>={n},64], got {tuple(kcache.shape)} / {tuple(vcache.shape)}")
            assert kcache.is_contiguous() and vcache.is_contiguous() and kcache.dtype == vcache.dtype == torch.bfloat16
        out = torch.empty((B, n, heads * 64), device=self.device, dtype=torch.bfloat16)
        opt = lambda t: _ptr(t) if t is not None else None
        self._check(lib.rdm_op_causal_attention_d64(self._h, _ptr(qkv), C3, B, n, heads, float(scale), _ptr(out), heads * 64, opt(kcache), opt(vcache), L))
        return out

    # ---- the RARM decode step's kernels one at a time
    def op_linear_rows(self, w, a=None, ln=None, bias=None, res_f32=None, out_bf16=None, out_f32=None, act=ACT_NONE, rows=None):
        """A linear op as the decode step calls it (one row per sequence, the context's current mode): act(A w^T + bias) (+ res_f32) with A =
        a (bf16 [M,K]) or LayerNorm(x; gamma, beta) for ln = (x f32 [M,K], gamma, beta).  out_bf16 / out_f32: tensors of at least `rows`
        rows to write into (out_f32 may BE res_f32: in place); neither given: a bf16 output is made.  -> (out_bf16, out_f32)."""
        if (a is None) == (ln is None):
            raise RdmError("op_linear_rows: exactly one of a (bf16 rows) and ln = (x, gamma, beta) required")
        src = a if a is not None else ln[0]
        M = src.shape[0] if rows is None else int(rows)
        K, N = src.shape[1], w.shape[0]
        No = N // 2 if act == ACT_GEGLU else N
        if tuple(w.shape) != (N, K) or w.dtype != torch.bfloat16 or src.dtype != (torch.bfloat16 if a is not None else torch.float32) or M < 1 or M > src.shape[0]:
            raise RdmError(f"op_linear_rows: operand [M >= {M},{K}] ({'bf16' if a is not None else 'f32'}) and w bf16 [{N},{K}] required, got {tuple(src.shape)} {src.dtype} / {tuple(w.shape)} {w.dtype}")
        if ln is not None:
            if res_f32 is not None or out_f32 is not None:
                raise RdmError("op_linear_rows: the LayerNorm form writes bf16 and takes no residual")
            if any(tuple(t.shape) != (K,) or t.dtype != torch.float32 for t in ln[1:]):
                raise RdmError(f"op_linear_rows: gamma and beta must be f32 [{K}]")
        if out_bf16 is None and out_f32 is None:
            out_bf16 = torch.empty((M, No), device=self.device, dtype=torch.bfloat16)
        for name, t, dt in (("out_bf16", out_bf16, torch.bfloat16), ("out_f32", out_f32, torch.float32), ("res_f32", res_f32, torch.float32)):
            if t is not None and (t.ndim != 2 or t.shape[0] < M or t.shape[1] != No or t.dtype != dt or not t.is_contiguous()):
                raise RdmError(f"op_linear_rows: {name} must be a contiguous {dt} [rows >= {M},{No}], got {tuple(t.shape)} {t.dtype}")
        if bias is not None and (tuple(bias.shape) != (N,) or bias.dtype != torch.float32):
            raise RdmError(f"op_linear_rows: bias must be f32 [{N}]")
        g, b = (ln[1], ln[2]) if ln is not None else (None, None)
        self._check(lib.rdm_op_linear_rows(self._h, _ptr(a), _ptr(ln[0]) if ln is not None else None, _ptr(g), _ptr(b), _ptr(w), _ptr(bias), _ptr(res_f32),
                                           _ptr(out_bf16), _ptr(out_f32), M, N, K, int(act)))
        return out_bf16, out_f32

    def op_rarm_decode_attention(self, q, kcache, vcache, heads, scale, pos=-1, k_new=None, v_new=None, nkv=None, out=None):
        """The decode step's attention at d_head 64 over a K/V cache.  q (and k_new / v_new) bf16 [B, heads*64] rows at one row stride (columns of
        a fused q | k | v projection are fine).  Caches bf16: [B, heads, L, 64] (head-major, the self-attention cache) or [B, rows, ld] views with
        the heads side by side in a row (the projected neighbours).  With k_new / v_new: they are stored at cache row pos and rows 0..pos
        attended; without: rows 0..nkv-1 (default: all of the cache's).  -> bf16 [B, heads*64]."""
        B, Cc = q.shape
        if Cc != heads * 64 or q.dtype != torch.bfloat16 or q.stride(1) != 1:
            raise RdmError(f"op_rarm_decode_attention: q must be bf16 [B,{heads * 64}] rows, got {tuple(q.shape)} {q.dtype}")
        if (k_new is None) != (v_new is None):
            raise RdmError("op_rarm_decode_attention: k_new and v_new come together")
        for t in (k_new, v_new):
            if t is not None and (tuple(t.shape) != (B, Cc) or t.dtype != torch.bfloat16 or t.stride(1) != 1 or t.stride(0) != q.stride(0)):
                raise RdmError(f"op_rarm_decode_attention: k_new / v_new must be bf16 [{B},{Cc}] rows at q's row stride")
        if kcache.shape != vcache.shape or kcache.stride() != vcache.stride() or kcache.dtype != torch.bfloat16 or vcache.dtype != torch.bfloat16 or kcache.ndim not in (3, 4):
            raise RdmError(f"op_rarm_decode_attention: caches must be two bf16 tensors of one shape, [B,heads,L,64] or [B,rows,ld], got {tuple(kcache.shape)} / {tuple(vcache.shape)}")
        if kcache.ndim == 4:
            if tuple(kcache.shape) != (B, heads, kcache.shape[2], 64) or not kcache.is_contiguous():
                raise RdmError(f"op_rarm_decode_attention: a head-major cache must be contiguous [{B},{heads},L,64], got {tuple(kcache.shape)}")
            cap, bs, rs, hs = kcache.shape[2], heads * kcache.shape[2] * 64, 64, kcache.shape[2] * 64
        else:
            if kcache.shape[0] != B or kcache.shape[2] != Cc or kcache.stride(2) != 1:
                raise RdmError(f"op_rarm_decode_attention: a row-major cache must be [{B},rows,{Cc}] rows, got {tuple(kcache.shape)}")
            cap, bs, rs, hs = kcache.shape[1], kcache.stride(0), kcache.stride(1), 0
        n = cap if nkv is None else int(nkv)
        if n < 1 or n > cap or n > 1024:
            raise RdmError(f"op_rarm_decode_attention: 1 <= nkv <= min(1024, the cache's {cap} rows) required, got {n}")
        pos = int(pos)
        if k_new is not None and not 0 <= pos < n:
            raise RdmError(f"op_rarm_decode_attention: 0 <= pos < {n} required with k_new / v_new, got {pos}")
        if k_new is None and pos < -1:
            raise RdmError(f"op_rarm_decode_attention: pos must be -1 (none) or a position, got {pos}")
        if out is None:
            out = torch.empty((B, Cc), device=self.device, dtype=torch.bfloat16)
        if tuple(out.shape) != (B, Cc) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise RdmError(f"op_rarm_decode_attention: out must be a contiguous bf16 [{B},{Cc}]")
        raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._check(lib.rdm_op_rarm_decode_attention(self._h, raw(q), q.stride(0), raw(k_new), raw(v_new), raw(kcache), raw(vcache), bs, rs, hs, n, pos,
                                                     float(scale), raw(out), Cc, heads, B))
        return out

    def op_rarm_xattn_decode(self, x, ln, G, UT, bias, heads, k, ln3=None, eps=1e-5):
        """The decode step's one-launch cross-attention, IN PLACE on x f32 [B2,C]: rows b < Bc get softmax_per_head(LayerNorm(x[b]; ln) G[b]^T) UT[b]
        + bias added, the others bias.  ln = (gamma, beta); G, UT bf16 [Bc,NP,C] (row h*k + j: head h, neighbour j); ln3 = (gamma, beta):
        -> bf16 [B2,C], LayerNorm of the finished rows (else None)."""
        if x.ndim != 2 or x.dtype != torch.float32 or not x.is_contiguous():
            raise RdmError(f"op_rarm_xattn_decode: x must be a contiguous f32 [B2,C], got {tuple(x.shape)} {x.dtype}")
        B2, Cc = x.shape
        if G.ndim != 3 or G.shape != UT.shape or G.shape[2] != Cc or G.dtype != torch.bfloat16 or UT.dtype != torch.bfloat16 or G.shape[0] > B2:
            raise RdmError(f"op_rarm_xattn_decode: G and UT must be bf16 [Bc <= {B2},NP,{Cc}], got {tuple(G.shape)} / {tuple(UT.shape)}")
        Bc, NP = G.shape[0], G.shape[1]
        if Cc % 8 or Cc > 1024 or heads < 1 or k < 1 or heads * k > min(128, NP):
            raise RdmError(f"op_rarm_xattn_decode: C a multiple of 8 up to 1024 and heads * k <= min(128, NP = {NP}) required, got C={Cc} heads={heads} k={k}")
        vecs = [ln[0], ln[1], bias] + (list(ln3) if ln3 is not None else [])
        if any(tuple(t.shape) != (Cc,) or t.dtype != torch.float32 for t in vecs):
            raise RdmError(f"op_rarm_xattn_decode: gamma, beta and bias must be f32 [{Cc}]")
        l3 = torch.empty((B2, Cc), device=self.device, dtype=torch.bfloat16) if ln3 is not None else None
        self._check(lib.rdm_op_rarm_xattn_decode(self._h, _ptr(x), _ptr(ln[0]), _ptr(ln[1]), float(eps), _ptr(G), _ptr(UT), _ptr(bias), B2, Bc, Cc, NP, heads, k,
                                                 _ptr(ln3[0]) if ln3 is not None else None, _ptr(ln3[1]) if ln3 is not None else None, _ptr(l3)))
        return l3

    def op_rarm_embed(self, tokens, emb, pos_t, pos=None, t=None, seq0=0, n_seq=None):
        """Token embedding + positional encoding -> f32 rows.  emb f32 [vocab,C], pos_t f32 [L,C]; ids outside [0, vocab) read row 0.
        pos given: the decode step, tokens int64 [B] -> [B,C] at position pos.  t given: the whole-sequence pass, tokens int64 [tok_rows,
        tok_ld >= t] -> [n_seq*t,C], sequence s reading token row (seq0 + s) % tok_rows (n_seq defaults to tok_rows)."""
        if (pos is None) == (t is None):
            raise RdmError("op_rarm_embed: exactly one of pos (decode step) and t (whole sequences) required")
        if emb.ndim != 2 or pos_t.ndim != 2 or emb.shape[1] != pos_t.shape[1] or emb.dtype != torch.float32 or pos_t.dtype != torch.float32 or tokens.dtype != torch.int64:
            raise RdmError("op_rarm_embed: emb f32 [vocab,C], pos_t f32 [L,C] and int64 tokens required")
        vocab, Cc = emb.shape
        L = pos_t.shape[0]
        if pos is not None:
            if tokens.ndim != 1 or not 0 <= int(pos) < L:
                raise RdmError(f"op_rarm_embed: tokens [B] and 0 <= pos < {L} required, got {tuple(tokens.shape)} / {pos}")
            rows, tt, ld, tr, p = tokens.shape[0], 1, 1, tokens.shape[0], int(pos)
        else:
            if tokens.ndim != 2 or not 1 <= int(t) <= min(L, tokens.shape[1]) or seq0 < 0:
                raise RdmError(f"op_rarm_embed: tokens [tok_rows, tok_ld >= t], 1 <= t <= {L} and seq0 >= 0 required, got {tuple(tokens.shape)} / t={t} seq0={seq0}")
            tr, ld = tokens.shape
            tt, p = int(t), -1
            rows = (tr if n_seq is None else int(n_seq)) * tt
        if rows < 1:
            raise RdmError("op_rarm_embed: no rows")
        x = torch.empty((rows, Cc), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_rarm_embed(self._h, _ptr(tokens), ld, tr, int(seq0), _ptr(emb), _ptr(pos_t), _ptr(x), rows, tt, Cc, vocab, L, p))
        return x

    def op_vq_attention(self, q, k, v, bias_v=None, scale=None):
        """The first stage's AttnBlock attention without its n x n scores: softmax(q k^T scale) v + bias_v over one head of C channels.
        q, k, v bf16 [B,n,C], each rows of C contiguous channels at one row stride (column blocks of a fused [B,n,3C] projection are fine);
        bias_v f32 [C] or None; scale defaults to C ** -0.5.  Any n >= 1, C a multiple of 128 up to 512 -> bf16 [B,n,C]."""
        B, n, Cc = q.shape
        if tuple(k.shape) != (B, n, Cc) or tuple(v.shape) != (B, n, Cc):
            raise RdmError(f"op_vq_attention: q, k, v must share one shape [B,n,C], got {tuple(q.shape)} / {tuple(k.shape)} / {tuple(v.shape)}")
        for t in (q, k, v):
            assert t.dtype == torch.bfloat16 and t.is_cuda
            if n > 0 and (t.stride(2) != 1 or (B > 1 and t.stride(0) != n * t.stride(1))):
                raise RdmError(f"op_vq_attention: rows of contiguous channels at one row stride required, got strides {t.stride()}")
        if bias_v is not None:
            bias_v = self._dev(bias_v, torch.float32).contiguous()
            if tuple(bias_v.shape) != (Cc,):
                raise RdmError(f"op_vq_attention: bias_v must be [{Cc}], got {tuple(bias_v.shape)}")
        out = torch.empty((B, n, Cc), device=self.device, dtype=torch.bfloat16)
        ld = lambda t: t.stride(1) if n > 0 else Cc
        raw = lambda t: C.c_void_p(t.data_ptr())           # views: _ptr() takes contiguous tensors only
        self._check(lib.rdm_op_vq_attention(self._h, raw(q), ld(q), raw(k), ld(k), raw(v), ld(v), _ptr(bias_v) if bias_v is not None else None, B, n, Cc,
                                            float(Cc ** -0.5 if scale is None else scale), _ptr(out), Cc))
        return out

    def op_rarm_nll(self, logits, targets):
        """logsumexp(logits) - logits[target] per row in fp32: logits f32 [rows,V] (V even), targets int64 [rows] -> f32 [rows]."""
        logits = self._dev(logits, torch.float32); targets = self._dev(targets, torch.int64)
        if logits.ndim != 2 or logits.shape[1] % 2 or tuple(targets.shape) != (logits.shape[0],):
            raise RdmError(f"op_rarm_nll: logits [rows, even V] and targets [rows] required, got {tuple(logits.shape)} / {tuple(targets.shape)}")
        self._check_ids("op_rarm_nll", targets, logits.shape[1], "targets")
        out = torch.empty((logits.shape[0],), device=self.device, dtype=torch.float32)
        self._check(lib.rdm_op_rarm_nll(self._h, _ptr(logits), logits.shape[0], logits.shape[1], _ptr(targets), _ptr(out)))
        return out

    def op_causal_attention_d64_bwd(self, qkv, out, dout, heads, scale):
        """Gradient of op_causal_attention_d64: qkv bf16 [B,n,3*heads*64], out (the forward's output) and dout bf16 [B,n,heads*64] ->
        dqkv bf16 [B,n,3*heads*64] = dq | dk | dv."""
        B, n, C3 = qkv.shape
        Cc = heads * 64
        assert qkv.dtype == out.dtype == dout.dtype == torch.bfloat16 and C3 == 3 * Cc
        if n < 1 or n > 1024:
            raise RdmError(f"op_causal_attention_d64_bwd: 1 <= n <= 1024 required, got {n}")
        if tuple(out.shape) != (B, n, Cc) or tuple(dout.shape) != (B, n, Cc):
            raise RdmError(f"op_causal_attention_d64_bwd: out and dout must be [{B},{n},{Cc}], got {tuple(out.shape)} / {tuple(dout.shape)}")
        dqkv = torch.empty((B, n, C3), device=self.device, dtype=torch.bfloat16)
        self._check(lib.rdm_op_causal_attention_d64_bwd(self._h, _ptr(qkv), C3, _ptr(out), Cc, _ptr(dout), Cc, B, n, heads, float(scale), _ptr(dqkv), C3))
        return dqkv

    def op_rarm_nll_bwd(self, logits, targets, gscale, want_nll=False, out=None, nll_out=None):
        """gscale * (softmax(logits) - onehot(targets)) as bf16 [rows,V]: logits f32 [rows,V] (V even), targets int64 [rows].
        want_nll: -> (dlogits, nll f32 [rows]), the second bitwise op_rarm_nll's.  out / nll_out: contiguous tensors to write into."""
        logits = self._dev(logits, torch.float32); targets = self._dev(targets, torch.int64)
        if logits.ndim != 2 or logits.shape[1] % 2 or tuple(targets.shape) != (logits.shape[0],):
            raise RdmError(f"op_rarm_nll_bwd: logits [rows, even V] and targets [rows] required, got {tuple(logits.shape)} / {tuple(targets.shape)}")
        self._check_ids("op_rarm_nll_bwd", targets, logits.shape[1], "targets")
        dl = out if out is not None else torch.empty(logits.shape, device=self.device, dtype=torch.bfloat16)
        nll = nll_out if nll_out is not None else (torch.empty((logits.shape[0],), device=self.device, dtype=torch.float32) if want_nll else None)
        assert dl.shape == logits.shape and dl.dtype == torch.bfloat16 and (nll is None or (nll.numel() == logits.shape[0] and nll.dtype == torch.float32))
        want_nll = want_nll or nll_out is not None
        self._check(lib.rdm_op_rarm_nll_bwd(self._h, _ptr(logits), logits.shape[0], logits.shape[1], _ptr(targets), float(gscale), _ptr(dl), _ptr(nll)))
        return (dl, nll) if want_nll else dl

    def op_embedding_grad(self, tokens, dy, V, out=None):
        """Gradient of an embedding lookup: tokens int64 [M], dy bf16 [M,C] -> f32 [V,C], row v the sum of dy[m] over tokens[m] == v
        (zero where the id is unused; `out` is overwritten whole)."""
        tokens = self._dev(tokens, torch.int64).reshape(-1)
        M, Cc = dy.shape
        if tokens.numel() != M or dy.dtype != torch.bfloat16:
            raise RdmError(f"op_embedding_grad: tokens [{M}] and dy bf16 [{M},{Cc}] required, got {tuple(tokens.shape)} / {dy.dtype}")
        self._check_ids("op_embedding_grad", tokens, V, "tokens")
        if out is None:
            out = torch.empty((V, Cc), device=self.device, dtype=torch.float32)
        assert tuple(out.shape) == (V, Cc) and out.dtype == torch.float32
        self._check(lib.rdm_op_embedding_grad(self._h, _ptr(tokens), _ptr(dy), M, Cc, V, _ptr(out)))
        return out

    def op_small_attention(self, q, k, v, heads, D, causal, scale, key_bias=None):
        """q [B, nq, >= heads D], k / v [B, nkv, >= heads D] bf16 at their real row strides: each may be a column slice of one fused
        [B, n, 3 heads D] projection (the CLIP towers' form), as long as a sample's rows follow the previous sample's at the same pitch."""
        B, nq, _ = q.shape

        def pitch(t):
            ld = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if B > 1 else t.shape[2])
            assert t.stride(2) == 1 and (B == 1 or t.stride(0) == t.shape[1] * ld), "rows of one pitch, samples back to back"
            return ld
        ldq, ldk, ldv = pitch(q), pitch(k), pitch(v)
        assert ldk == ldv, "k and v share one row pitch"
        out = torch.empty((B, nq, heads * D), device=self.device, dtype=torch.bfloat16)
        p = lambda t: C.c_void_p(t.data_ptr())
        if key_bias is not None:      # fp32 [B, nkv], added to every head's scaled score of key j; -inf keys are skipped
            kb = self._key_bias("op_small_attention", key_bias, B, k.shape[1])
            self._check(lib.rdm_op_small_attention_biased(self._h, p(q), ldq, p(k), p(v), ldk, B, nq, k.shape[1], heads,
                                                          D, int(causal), float(scale), _ptr(out), heads * D, _ptr(kb)))
            return out
        self._check(lib.rdm_op_small_attention(self._h, p(q), ldq, p(k), p(v), ldk, B, nq, k.shape[1], heads,
                                               D, int(causal), float(scale), _ptr(out), heads * D))
        return out
