"""ctypes binding of ``csrc/libpdengine.so`` (C ABI: ``include/pdengine.h``).

There is no CPU fallback: if the HIP library is missing, or no MI355X is visible,
construction raises.  Arrays cross the boundary as float32 in the reference's layouts
(NCHW latents/images, [B, L, D] context); NumPy arrays are passed as host pointers,
torch CUDA tensors as device pointers.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .weights import (CLIP_VIT_H14, CLIP_VIT_L14_SAFETY, IMAGE_ENCODER_PREFIX, SAFETY_PREFIX, ClipVisionConfig, ModelConfig, SD15,  # noqa: F401
                      clip_vision_param_shapes, fold_mlsd_state_dict, hed_key, safety_param_shapes)

PD_PREC_BF16, PD_PREC_F32, PD_PREC_F16, PD_PREC_F16X2 = 0, 1, 2, 3
PRECISIONS = {"bf16": PD_PREC_BF16, "f32": PD_PREC_F32, "fp32": PD_PREC_F32, "f16": PD_PREC_F16, "fp16": PD_PREC_F16,
              "f16x2": PD_PREC_F16X2}
PD_MEM_HOST, PD_MEM_DEVICE = 0, 1
PD_DT_F32, PD_DT_F16, PD_DT_BF16 = 0, 1, 2
PD_GET_LATENTS, PD_GET_PRED_X0, PD_GET_EPS = 0, 1, 2
PD_VAE_MEAN, PD_VAE_SAMPLE, PD_VAE_MOMENTS = 0, 1, 2
VAE_ENCODE_MODES = {"mean": PD_VAE_MEAN, "sample": PD_VAE_SAMPLE, "moments": PD_VAE_MOMENTS}
PD_HED_EDGE, PD_HED_SIDES = 0, 1
HED_OUTPUTS = {"edge": PD_HED_EDGE, "sides": PD_HED_SIDES}
PD_MLSD_TPMAP, PD_MLSD_SEGMENTS, PD_MLSD_LINES = 0, 1, 2
MLSD_OUTPUTS = {"tpmap": PD_MLSD_TPMAP, "segments": PD_MLSD_SEGMENTS, "lines": PD_MLSD_LINES}
MLSD_TOPK = 200
# image ends (include/pdengine.h, "Image ends"): the filters carry PIL's own numbers
PD_RESAMPLE_LANCZOS, PD_RESAMPLE_BOX = 1, 4
PD_RESAMPLE_MAX_SCALE = 8
RESAMPLE_FILTERS = {"lanczos": PD_RESAMPLE_LANCZOS, "box": PD_RESAMPLE_BOX}
# ... plus PIL.Image.BICUBIC, for pd_resample_coefficients_ex and the CLIP preprocessing only (pd_image_load keeps its two)
PD_RESAMPLE_BICUBIC = 3
RESAMPLE_FILTERS_EX = dict(RESAMPLE_FILTERS, bicubic=PD_RESAMPLE_BICUBIC)
# CLIP image tower (include/pdengine.h, "CLIP image tower")
PD_CLIP_OUT_PIXEL_VALUES, PD_CLIP_OUT_PATCHES, PD_CLIP_OUT_BYTES = 0, 1, 2
CLIP_PREPROCESS_OUTPUTS = {"pixel_values": PD_CLIP_OUT_PIXEL_VALUES, "patches": PD_CLIP_OUT_PATCHES, "bytes": PD_CLIP_OUT_BYTES}
PD_CLIP_IN_U8, PD_CLIP_IN_PIXEL_VALUES = 0, 1
PD_CLIP_ACT_QUICK_GELU, PD_CLIP_ACT_GELU = 0, 1
CLIP_ACTS = {"quick_gelu": PD_CLIP_ACT_QUICK_GELU, "gelu": PD_CLIP_ACT_GELU}
CLIP_VISION_OUTPUTS = ("embeds", "pooled", "hidden")
PD_SAFETY_CONCEPTS, PD_SAFETY_SPECIAL = 17, 3
PD_IMAGE_REPEAT, PD_IMAGE_TILE = 0, 1
IMAGE_BATCH_MODES = {"repeat": PD_IMAGE_REPEAT, "tile": PD_IMAGE_TILE}
PD_ROUND_NEAREST_EVEN, PD_ROUND_TRUNC = 0, 1
IMAGE_ROUNDINGS = {"nearest_even": PD_ROUND_NEAREST_EVEN, "trunc": PD_ROUND_TRUNC}
PD_MAX_LEVELS = 8
PD_NUM_CONTROL = 13
PD_MAX_CONTEXT_LEN = 1024
PD_COMM_ID_BYTES = 128

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libpdengine.so")


class PdError(RuntimeError):
    pass


class pd_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("hint_channels", C.c_int32),
        ("query_channels", C.c_int32), ("model_channels", C.c_int32), ("num_levels", C.c_int32),
        ("channel_mult", C.c_int32 * PD_MAX_LEVELS), ("num_res_blocks", C.c_int32),
        ("num_attn_res", C.c_int32), ("attention_resolutions", C.c_int32 * PD_MAX_LEVELS),
        ("num_heads", C.c_int32), ("context_dim", C.c_int32), ("context_len", C.c_int32),
        ("hint_widths", C.c_int32 * 7), ("timesteps", C.c_int32), ("linear_start", C.c_double),
        ("linear_end", C.c_double), ("precision", C.c_int32), ("stream_f32", C.c_int32),
        ("vae_ch", C.c_int32), ("vae_num_levels", C.c_int32), ("vae_ch_mult", C.c_int32 * PD_MAX_LEVELS),
        ("vae_num_res_blocks", C.c_int32), ("vae_out_ch", C.c_int32), ("scale_factor", C.c_double),
        ("text_vocab", C.c_int32), ("text_layers", C.c_int32), ("text_heads", C.c_int32), ("text_ff", C.c_int32),
        ("vae_encoder", C.c_int32), ("reserved", C.c_int32 * 1),
    ]


class _ContextLen(C.Union):
    """pd_sample_args.context_len; `reserved` is the field's name before it had a meaning, kept as an alias of the same four bytes"""
    _fields_ = [("context_len", C.c_int32), ("reserved", C.c_int32 * 1)]


class pd_sample_args(C.Structure):
    _anonymous_ = ("_ctx",)
    _fields_ = [
        ("batch", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("steps", C.c_int32),
        ("eta", C.c_float), ("cfg_scale", C.c_float), ("use_cfg", C.c_int32), ("guess_mode", C.c_int32),
        ("only_mid_control", C.c_int32), ("temperature", C.c_float), ("mem", C.c_int32),
        ("x_T", C.c_void_p), ("ctx_cond", C.c_void_p), ("ctx_uncond", C.c_void_p), ("pair", C.c_void_p),
        ("query", C.c_void_p), ("pair_uncond", C.c_void_p), ("query_uncond", C.c_void_p),
        ("control_scales", C.c_void_p), ("control_scales_step", C.c_void_p), ("noise", C.c_void_p),
        ("timesteps", C.c_void_p), ("init_latents", C.c_void_p), ("mask", C.c_void_p), ("init_flags", C.c_int32),
        ("_ctx", _ContextLen),
    ]


PD_INIT_PURE_NOISE, PD_NOISE_FROM_SEED, PD_XT_FROM_SEED = 1, 2, 4
# streams of the engine's seeded generator (include/pdengine.h, "Seeded noise")
PD_RNG_XT, PD_RNG_STEP, PD_RNG_VAE, PD_RNG_USER = 0, 1, 2, 16
RNG_STREAMS = {"xt": PD_RNG_XT, "step": PD_RNG_STEP, "vae": PD_RNG_VAE}


class pd_unipc_args(C.Structure):
    _fields_ = [
        ("order", C.c_int32), ("bh2", C.c_int32), ("lower_order_final", C.c_int32), ("n_disable_corrector", C.c_int32),
        ("disable_corrector", C.c_void_p), ("reserved", C.c_int32 * 4),
    ]


PD_UNIPC_NCOEF = 16


class pd_image_load_args(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("Bs", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("mem_src", C.c_int32),
        ("dst", C.c_void_p), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("c_off", C.c_int32),
        ("mem_dst", C.c_int32), ("filter", C.c_int32), ("batch_mode", C.c_int32), ("mul", C.c_float), ("add", C.c_float),
        ("reserved", C.c_int32 * 4),
    ]


class pd_clip_preprocess_args(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("mem_src", C.c_int32), ("image_size", C.c_int32),
        ("patch", C.c_int32), ("out_mode", C.c_int32), ("mem_dst", C.c_int32), ("dst", C.c_void_p), ("mean", C.c_float * 3),
        ("std", C.c_float * 3), ("reserved", C.c_int32 * 4),
    ]


class pd_clip_vision_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden", "layers", "heads", "ff", "patch", "image_size", "proj_dim", "act")] + \
               [("eps", C.c_float), ("stream_f32", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("prefix", C.c_char * 64),
                ("reserved", C.c_int32 * 4)]


class pd_clip_vision_args(C.Structure):
    _fields_ = [("prefix", C.c_char_p), ("input", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("input_kind", "B", "H", "W", "mem", "hidden_layer")] + \
               [("image_embeds", C.c_void_p), ("pooler_output", C.c_void_p), ("hidden", C.c_void_p), ("reserved", C.c_int64 * 2)]


class pd_ip_adapter_config(C.Structure):
    _fields_ = [("num_tokens", C.c_int32), ("embed_dim", C.c_int32), ("reserved", C.c_int32 * 6)]


class pd_mlsd_args(C.Structure):
    _fields_ = [("images", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("mem", C.c_int32), ("what", C.c_int32),
                ("thr_v", C.c_float), ("thr_d", C.c_float), ("out", C.c_void_p), ("dst_f", C.c_void_p), ("mem_f", C.c_int32),
                ("Cf", C.c_int32), ("c_off", C.c_int32), ("mul", C.c_float), ("add", C.c_float)]


PD_LORA_PAIR, PD_LORA_HADA, PD_LORA_KRON = 0, 1, 2
LORA_KINDS = {"pair": PD_LORA_PAIR, "hada": PD_LORA_HADA, "kron": PD_LORA_KRON}


class LoraFactors(C.Structure):   # pd_lora_factors
    _fields_ = [("kind", C.c_int32), ("rank", C.c_int32), ("rank2", C.c_int32), ("kron_a", C.c_int32), ("kron_b", C.c_int32),
                ("scale", C.c_float), ("up", C.c_void_p), ("down", C.c_void_p), ("up2", C.c_void_p), ("down2", C.c_void_p),
                ("magnitude", C.c_void_p)]


class pd_canny_args(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("mem_src", C.c_int32),
        ("low", C.c_float), ("high", C.c_float), ("dst_u8", C.c_void_p), ("mem_u8", C.c_int32), ("Cf", C.c_int32),
        ("c_off", C.c_int32), ("dst_f", C.c_void_p), ("mul", C.c_float), ("add", C.c_float), ("mem_f", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class pd_lms_args(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("order", C.c_int32), ("solver_type", C.c_int32), ("lower_order_final", C.c_int32),
        ("model_times", C.c_void_p), ("rows", C.c_void_p), ("row_times", C.c_void_p), ("n_rows", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


PD_LMS_NCOEF = 16
PD_LMS_PLMS, PD_LMS_DPMPP, PD_LMS_ROWS, PD_LMS_EULER_A = 0, 1, 2, 3
PD_LMS_F_DATA_PRED, PD_LMS_F_BASE_KEEP, PD_LMS_F_STORE_KEEP, PD_LMS_F_PUSH, PD_LMS_F_STEP = 1, 2, 4, 8, 16
_LMS_KINDS = {"plms": PD_LMS_PLMS, "dpmsolver++": PD_LMS_DPMPP, "rows": PD_LMS_ROWS, "euler_a": PD_LMS_EULER_A}
# DPM_Solver's names and the names diffusers gives the same two second-order updates
_LMS_SOLVER_TYPES = {"dpm_solver": 0, "dpmsolver": 0, "midpoint": 0, "taylor": 1, "heun": 1}

_lib = None


def _torch_runtime_first():
    """PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) under the same soname as the system one that
    libpdengine.so links.  The dynamic loader keeps whichever is loaded first for the whole process: with the system
    runtime first, torch (built against its own) later reports "No HIP GPUs are available"; with torch's first, both
    work.  So when torch is installed, load it -- and bring its device runtime up -- before libpdengine.so is opened.
    CUDA tensors can then be handed to the engine as device pointers whatever the caller's import order."""
    try:
        import torch
    except ImportError:
        return
    try:
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:   # noqa: BLE001 - torch without a usable device: the engine reports the real error
        pass


class pd_gemm_ex_args(C.Structure):
    """include/pdengine_ops.h"""
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "bias", "residual", "rowvec", "gate", "ln_gamma", "ln_beta")] + \
               [(n, C.c_int32) for n in ("M", "K", "N", "act", "a_silu", "res_dt", "out_dt", "rows_per_sample", "vt_begin", "vt_extra", "vt_tok_off",
                                         "c_sample_rows", "c_row_off", "a_sample_rows", "a_row_off", "ldc_extra")] + \
               [("scale", C.c_float), ("y", C.c_void_p), ("vt", C.c_void_p), ("touched", C.c_int64)]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libpdengine.so and declare the prototypes of include/pdengine.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("PDENGINE_LIB") or LIB_PATH    # PDENGINE_LIB: A/B another build of the library
    if not os.path.exists(p):
        raise PdError(f"{p} not found: build it with `make -C {_CSRC}` (or __graft_entry__.build()); "
                      "pdengine has no CPU fallback")
    _torch_runtime_first()
    lib = C.CDLL(p)
    lib.pd_last_error.restype = C.c_char_p
    lib.pd_abi_version.restype = C.c_int
    lib.pd_engine_create.argtypes = [C.POINTER(pd_config), C.c_int, C.POINTER(C.c_void_p)]
    lib.pd_engine_destroy.argtypes = [C.c_void_p]
    lib.pd_engine_destroy.restype = None
    lib.pd_param_count.argtypes = [C.c_void_p]
    lib.pd_param_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.pd_load_weights.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32]
    lib.pd_init_random_weights.argtypes = [C.c_void_p, C.c_uint64]
    lib.pd_weights_missing.argtypes = [C.c_void_p]
    lib.pd_vae_weights_missing.argtypes = [C.c_void_p]
    lib.pd_vae_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.pd_vae_encode.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]
    lib.pd_vae_encoder_weights_missing.argtypes = [C.c_void_p]
    lib.pd_vae_set_tiling.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32]
    lib.pd_vae_set_slicing.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.pd_vae_get_tiling.argtypes = [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 3 + [C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.pd_vae_tile_plan.argtypes = [C.c_int32] * 3 + [C.c_double, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 3 + [C.c_void_p, C.c_int32]
    lib.pd_op_vae_tile_blend.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p]
    lib.pd_hed_configure.argtypes = [C.c_void_p]
    lib.pd_hed_weights_missing.argtypes = [C.c_void_p]
    lib.pd_hed_detect.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p]
    lib.pd_text_weights_missing.argtypes = [C.c_void_p]
    lib.pd_text_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.pd_text_encode_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.pd_eps.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
    lib.pd_eps_ctx.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
    lib.pd_control_shape.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 3
    lib.pd_ddim_sample.argtypes = [C.c_void_p, C.POINTER(pd_sample_args), C.c_int32, C.c_void_p, C.c_void_p]
    lib.pd_sample_begin.argtypes = [C.c_void_p, C.POINTER(pd_sample_args)]
    lib.pd_sample_step.argtypes = [C.c_void_p, C.c_int32]
    lib.pd_sample_get.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.pd_sample_set_latents.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.pd_sample_eps_at.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.pd_sample_set_guidance.argtypes = [C.c_void_p, C.c_float]
    lib.pd_sample_end.argtypes = [C.c_void_p]
    lib.pd_make_schedule.argtypes = [C.c_void_p, C.c_int32, C.c_float] + [C.c_void_p] * 5
    lib.pd_unipc_coefficients.argtypes = [C.POINTER(pd_config), C.POINTER(pd_unipc_args), C.c_void_p, C.c_int32, C.c_void_p]
    lib.pd_unipc_sample.argtypes = [C.c_void_p, C.POINTER(pd_sample_args), C.POINTER(pd_unipc_args), C.c_int32, C.c_void_p,
                                    C.c_void_p]
    lib.pd_sample_begin_unipc.argtypes = [C.c_void_p, C.POINTER(pd_sample_args), C.POINTER(pd_unipc_args)]
    lib.pd_lms_coefficients.argtypes = [C.POINTER(pd_config), C.POINTER(pd_lms_args), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int32)]
    lib.pd_lms_sample.argtypes = [C.c_void_p, C.POINTER(pd_sample_args), C.POINTER(pd_lms_args), C.c_int32, C.c_void_p, C.c_void_p]
    lib.pd_sample_begin_lms.argtypes = [C.c_void_p, C.POINTER(pd_sample_args), C.POINTER(pd_lms_args)]
    lib.pd_sample_rows.argtypes = [C.c_void_p]
    lib.pd_sample_rows.restype = C.c_int32
    lib.pd_synchronize.argtypes = [C.c_void_p]
    lib.pd_stream.argtypes = [C.c_void_p]
    lib.pd_stream.restype = C.c_void_p
    lib.pd_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.pd_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    if hasattr(lib, "pd_get_option"):   # (an older build handed in through PDENGINE_LIB for an A/B run lacks the two)
        lib.pd_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
        lib.pd_option_info.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    lib.pd_comm_new_id.argtypes = [C.c_void_p]
    lib.pd_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.pd_comm_world.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.pd_comm_all_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.pd_comm_destroy.argtypes = [C.c_void_p]
    lib.pd_get_stat.argtypes = [C.c_void_p, C.c_char_p]
    lib.pd_get_stat.restype = C.c_int64
    lib.pd_bench_conv3x3.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.POINTER(C.c_float)]
    lib.pd_bench_linear.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_float)]
    lib.pd_profile_dump.argtypes = [C.c_void_p, C.c_char_p]
    lib.pd_profile_read.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    # per-op parity hooks (include/pdengine_ops.h)
    fp = C.c_void_p
    lib.pd_op_conv2d.argtypes = [C.c_void_p, fp, fp, fp, fp] + [C.c_int] * 9 + [C.c_float, C.c_int, fp]
    if hasattr(lib, "pd_op_conv2d_upfold"):   # (an older build handed in through PDENGINE_LIB for an A/B run lacks it)
        lib.pd_op_conv2d_upfold.argtypes = [C.c_void_p, fp, fp, fp, fp] + [C.c_int] * 5 + [fp]
    lib.pd_op_linear.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 5 + [fp]
    if hasattr(lib, "pd_op_linear_ex"):
        lib.pd_op_linear_ex.argtypes = [C.c_void_p, C.POINTER(pd_gemm_ex_args)]
        lib.pd_op_conv2d_ex.argtypes = [C.c_void_p, fp, fp, fp, fp, fp] + [C.c_int] * 9 + [C.c_float, C.c_int, fp]
    lib.pd_op_linear_fp8.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [fp]
    lib.pd_op_groupnorm.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [C.c_float, C.c_int, fp]
    lib.pd_op_layernorm.argtypes = [C.c_void_p, fp, fp, fp, C.c_int, C.c_int, fp]
    lib.pd_op_groupnorm_slabs.argtypes = [C.c_void_p, fp, C.c_int, fp, fp, fp, fp] + [C.c_int] * 4 + [C.c_float, C.c_int, fp]
    lib.pd_op_groupnorm_coef.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [C.c_float, fp]
    lib.pd_op_ln_linear.argtypes = [C.c_void_p, C.c_int] + [fp] * 9 + [C.c_int] * 3 + [fp, fp, C.POINTER(C.c_int), fp]
    lib.pd_op_attention.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [fp]
    lib.pd_op_attention_ex.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 6 + [C.c_float, fp, C.c_int, C.c_int, C.c_float, fp, C.POINTER(C.c_int64)]
    lib.pd_op_vae_attention.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 3 + [fp]
    lib.pd_bench_vae_attention.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    lib.pd_op_spatial_transformer.argtypes = [C.c_void_p, C.c_char_p, fp, fp] + [C.c_int] * 3 + [fp]
    lib.pd_op_spatial_transformer_ctx.argtypes = [C.c_void_p, C.c_char_p, fp, fp] + [C.c_int] * 4 + [fp]
    lib.pd_op_time_embed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, fp, fp]
    lib.pd_op_vae_downsample.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [fp]
    lib.pd_op_hed_stage_tail.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [fp, fp]
    lib.pd_op_hed_fuse.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 4 + [fp]
    lib.pd_read_weights.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.pd_lora_add.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                C.POINTER(C.c_int64), C.c_int32]
    lib.pd_lora_add_ex.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.POINTER(LoraFactors)]
    lib.pd_lora_set_scales.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.pd_lora_remove.argtypes = [C.c_void_p, C.c_int32]
    lib.pd_set_freeu.argtypes = [C.c_void_p] + [C.c_float] * 4
    lib.pd_get_freeu.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.pd_op_freeu_concat.argtypes = [C.c_void_p, fp, fp, fp, fp] + [C.c_int] * 7 + [C.c_float, C.c_float, fp]
    lib.pd_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
    lib.pd_philox4x32_10.restype = None
    lib.pd_set_rng.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    lib.pd_get_rng.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.pd_randn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]
    lib.pd_resample_coefficients.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    lib.pd_image_load.argtypes = [C.c_void_p, C.POINTER(pd_image_load_args)]
    if hasattr(lib, "pd_clip_vision_configure"):   # (an older build handed in through PDENGINE_LIB for an A/B run lacks the image tower)
        lib.pd_resample_coefficients_ex.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
        lib.pd_clip_preprocess.argtypes = [C.c_void_p, C.POINTER(pd_clip_preprocess_args)]
        lib.pd_clip_preprocess_geometry.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 4
        lib.pd_clip_patch_width.argtypes = [C.c_int32]
        lib.pd_clip_vision_configure.argtypes = [C.c_void_p, C.POINTER(pd_clip_vision_config)]
        lib.pd_clip_vision_weights_missing.argtypes = [C.c_void_p, C.c_char_p]
        lib.pd_clip_vision_forward.argtypes = [C.c_void_p, C.POINTER(pd_clip_vision_args)]
        lib.pd_safety_configure.argtypes = [C.c_void_p]
        lib.pd_safety_weights_missing.argtypes = [C.c_void_p]
        lib.pd_safety_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.pd_safety_blank.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_float]
    if hasattr(lib, "pd_ip_adapter_configure"):   # (as above: an older build lacks the adapter)
        lib.pd_ip_adapter_configure.argtypes = [C.c_void_p, C.POINTER(pd_ip_adapter_config)]
        lib.pd_ip_adapter_weights_missing.argtypes = [C.c_void_p]
        lib.pd_ip_adapter_set_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.pd_ip_adapter_get_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.pd_ip_adapter_set_image.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        lib.pd_ip_adapter_clear_image.argtypes = [C.c_void_p]
        lib.pd_bench_ip_attention.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_float)] * 2
        lib.pd_op_ip_attention_add.argtypes = [C.c_void_p, fp, fp, fp, fp] + [C.c_int] * 6 + [C.c_float, C.c_float, fp]
        lib.pd_op_spatial_transformer_ip.argtypes = [C.c_void_p, C.c_char_p, fp, fp, fp] + [C.c_int] * 5 + [fp]
    if hasattr(lib, "pd_set_pag"):   # (as above: an older build lacks perturbed-attention guidance)
        lib.pd_set_pag.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32]
        lib.pd_get_pag.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        lib.pd_bench_pag_identity.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(C.c_float)] * 2
        lib.pd_op_pag_identity.argtypes = [C.c_void_p, fp] + [C.c_int] * 5 + [fp]
        lib.pd_op_cfg_combine.argtypes = [C.c_void_p, fp] + [C.c_int] * 5 + [C.c_float, C.c_float, fp]
        lib.pd_op_spatial_transformer_pag.argtypes = [C.c_void_p, C.c_char_p, fp, fp] + [C.c_int] * 5 + [fp]
    lib.pd_image_store.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_int32]
    lib.pd_canny.argtypes = [C.c_void_p, C.POINTER(pd_canny_args)]
    lib.pd_op_canny_hysteresis.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.pd_mlsd_configure.argtypes = [C.c_void_p]
    lib.pd_mlsd_weights_missing.argtypes = [C.c_void_p]
    lib.pd_mlsd_detect.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_float, C.c_float, C.c_void_p]
    lib.pd_mlsd_detect_ex.argtypes = [C.c_void_p, C.POINTER(pd_mlsd_args)]
    lib.pd_op_dwconv3x3.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 6 + [fp]
    lib.pd_op_upcat_bilinear.argtypes = [C.c_void_p, fp] + [C.c_int] * 6 + [fp]
    lib.pd_op_conv2d_dilated.argtypes = [C.c_void_p, fp, fp, fp] + [C.c_int] * 7 + [fp]
    lib.pd_op_mlsd_decode.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.pd_op_draw_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    lib.pd_op_sd3_update.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p] * 2
    if path is None:
        _lib = lib
    return lib


EXPORTS = [
    "pd_last_error", "pd_abi_version", "pd_engine_create", "pd_engine_destroy", "pd_param_count", "pd_param_info",
    "pd_load_weights", "pd_init_random_weights", "pd_weights_missing", "pd_vae_weights_missing", "pd_vae_decode",
    "pd_vae_encode", "pd_vae_encoder_weights_missing", "pd_vae_set_tiling", "pd_vae_set_slicing", "pd_vae_get_tiling", "pd_vae_tile_plan",
    "pd_op_vae_tile_blend", "pd_eps", "pd_eps_ctx", "pd_control_shape", "pd_ddim_sample",
    "pd_sample_begin", "pd_sample_step", "pd_sample_get", "pd_sample_set_latents", "pd_sample_set_guidance", "pd_sample_eps_at", "pd_sample_end",
    "pd_unipc_coefficients", "pd_unipc_sample", "pd_sample_begin_unipc",
    "pd_lms_coefficients", "pd_lms_sample", "pd_sample_begin_lms", "pd_sample_rows",
    "pd_make_schedule", "pd_synchronize", "pd_stream", "pd_wait_stream", "pd_set_option", "pd_get_option", "pd_option_info", "pd_get_stat", "pd_bench_conv3x3", "pd_bench_linear", "pd_text_encode", "pd_text_encode_ex", "pd_text_weights_missing",
    "pd_profile_read", "pd_profile_dump", "pd_comm_new_id", "pd_comm_init", "pd_comm_world", "pd_comm_all_gather", "pd_comm_destroy",
    "pd_sd3_configure", "pd_sd3_weights_missing", "pd_sd3_forward", "pd_sd3_control", "pd_sd3_sample", "pd_sd3_sample_ex", "pd_sd3_down_proj",
    "pd_op_sd3_update",
    "pd_op_conv2d", "pd_op_conv2d_ex", "pd_op_conv2d_upfold", "pd_op_linear", "pd_op_linear_ex", "pd_op_linear_fp8", "pd_op_groupnorm", "pd_op_layernorm", "pd_op_groupnorm_slabs", "pd_op_groupnorm_coef", "pd_op_ln_linear", "pd_op_attention", "pd_op_attention_ex", "pd_op_spatial_transformer", "pd_op_spatial_transformer_ctx", "pd_op_time_embed",
    "pd_op_timestep_embedding_i", "pd_op_timestep_embedding_f", "pd_op_vae_downsample", "pd_read_weights", "pd_lora_add", "pd_lora_add_ex", "pd_lora_set_scales", "pd_lora_remove",
    "pd_set_freeu", "pd_get_freeu", "pd_op_freeu_concat",
    "pd_philox4x32_10", "pd_set_rng", "pd_get_rng", "pd_randn",
    "pd_hed_configure", "pd_hed_weights_missing", "pd_hed_detect", "pd_op_hed_stage_tail", "pd_op_hed_fuse",
    "pd_mlsd_configure", "pd_mlsd_weights_missing", "pd_mlsd_detect", "pd_mlsd_detect_ex", "pd_op_dwconv3x3", "pd_op_upcat_bilinear", "pd_op_conv2d_dilated",
    "pd_op_mlsd_decode", "pd_op_draw_lines",
    "pd_resample_coefficients", "pd_image_load", "pd_image_store", "pd_canny", "pd_op_canny_hysteresis",
    "pd_sd3_text_configure", "pd_sd3_text_weights_missing", "pd_sd3_encode_prompt", "pd_sd3_text_encoder", "pd_t5_relative_buckets",
    "pd_resample_coefficients_ex", "pd_clip_preprocess", "pd_clip_preprocess_geometry", "pd_clip_patch_width", "pd_clip_vision_configure",
    "pd_clip_vision_weights_missing", "pd_clip_vision_forward", "pd_safety_configure", "pd_safety_weights_missing", "pd_safety_check", "pd_safety_blank",
    "pd_ip_adapter_configure", "pd_ip_adapter_weights_missing", "pd_ip_adapter_set_scale", "pd_ip_adapter_get_scale", "pd_ip_adapter_set_image",
    "pd_ip_adapter_clear_image", "pd_bench_ip_attention", "pd_op_ip_attention_add", "pd_op_spatial_transformer_ip",
    "pd_set_pag", "pd_get_pag", "pd_bench_pag_identity", "pd_op_pag_identity", "pd_op_cfg_combine", "pd_op_spatial_transformer_pag",
    "pd_sd3_vae_configure", "pd_sd3_vae_weights_missing", "pd_sd3_vae_config_layout", "pd_sd3_vae_decode", "pd_sd3_vae_encode", "pd_op_vae_attention", "pd_bench_vae_attention",
]


def option_table() -> List[Tuple[str, int]]:
    """(key, default) of every engine option, in the order of the engine's table (pd_option_info; host only, no engine)."""
    lib = load_library()
    rows, k, d = [], C.c_char_p(), C.c_int64()
    while not lib.pd_option_info(len(rows), C.byref(k), C.byref(d)):
        rows.append((k.value.decode(), int(d.value)))
    return rows


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """One Philox4x32-10 block on the host (pd_philox4x32_10): the generator behind Engine.randn and the in-kernel draws."""
    lib = load_library()
    c = (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in counter])
    k = (C.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in key])
    out = (C.c_uint32 * 4)()
    lib.pd_philox4x32_10(c, k, out)
    return tuple(int(v) for v in out)


def _filter_code(filter) -> int:
    return RESAMPLE_FILTERS[filter] if isinstance(filter, str) else int(filter)


PD_VAE_SD15, PD_VAE_SD3 = 0, 1
VAE_TILE_DEFAULTS = {PD_VAE_SD15: 64, PD_VAE_SD3: 128}   # tile_latent; overlap_factor 0.25 for both


class pd_vae_tile(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("y0", "x0", "h", "w", "oy", "ox", "oh", "ow", "th", "tw", "ev", "eh", "cls")] + [("reserved", C.c_int32 * 3)]


VaeTile = collections.namedtuple("VaeTile", "y0 x0 h w oy ox oh ow th tw ev eh cls")
VaeTilePlan = collections.namedtuple("VaeTilePlan", "rows cols classes tiles")
VaeTilingState = collections.namedtuple("VaeTilingState", "tiling slicing tile_latent overlap_factor tile_batch")


def vae_tile_plan(h: int, w: int, tile_latent: int = 64, overlap_factor: float = 0.25, u: int = 8, encode: bool = False) -> VaeTilePlan:
    """The tile grid of a tiled VAE call (pd_vae_tile_plan; host only, no engine): diffusers' tiled_decode on a latent of h x w, or with
    encode=True tiled_encode on an image of h x w pixels.  rows = cols = 0 and no tiles when the size is not tiled; tiles in row-major
    order (input window, kept output rectangle, the tile's own output size, blend extents, shape class).  PdError for an overlap_factor
    outside (0, 1/3] or a tile_latent * overlap_factor that is no integer."""
    lib = load_library()
    r, c, k = C.c_int32(), C.c_int32(), C.c_int32()
    args = (int(h), int(w), int(tile_latent), float(overlap_factor), int(u), int(bool(encode)))
    if lib.pd_vae_tile_plan(*args, C.byref(r), C.byref(c), C.byref(k), None, 0):
        raise PdError(lib.pd_last_error().decode())
    n = r.value * c.value
    buf = (pd_vae_tile * max(n, 1))()
    if n and lib.pd_vae_tile_plan(*args, C.byref(r), C.byref(c), C.byref(k), C.addressof(buf), n):
        raise PdError(lib.pd_last_error().decode())
    return VaeTilePlan(r.value, c.value, k.value, [VaeTile(*(getattr(buf[i], f) for f in VaeTile._fields)) for i in range(n)])


def resample_ksize(in_size: int, out_size: int, filter="lanczos") -> int:
    """Taps per output of Pillow's 8-bit resampler along one axis (pd_resample_coefficients' size query); PdError for a
    reduction beyond PD_RESAMPLE_MAX_SCALE or an unknown filter."""
    lib = load_library()
    ks = C.c_int32()
    if lib.pd_resample_coefficients(int(in_size), int(out_size), _filter_code(filter), C.byref(ks), None, None):
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    return int(ks.value)


def resample_coefficients(in_size: int, out_size: int, filter="lanczos") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds [out_size, 2] = (xmin, count), kk [out_size, ksize], zero padded; both int32): the tables of Pillow's 8-bit
    Image.resize along one axis (pd_resample_coefficients; host only, no engine).  filter: "lanczos" / "box" or PIL's number."""
    lib = load_library()
    ks = C.c_int32(resample_ksize(in_size, out_size, filter))
    bounds = np.zeros((int(out_size), 2), np.int32)
    kk = np.zeros((int(out_size), ks.value), np.int32)
    if lib.pd_resample_coefficients(int(in_size), int(out_size), _filter_code(filter), C.byref(ks), bounds.ctypes.data, kk.ctypes.data):
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    return bounds, kk


def resample_coefficients_ex(in_size: int, out_size: int, filter="bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """resample_coefficients with PIL.Image.BICUBIC accepted as well (pd_resample_coefficients_ex): "lanczos" / "box" / "bicubic" or
    PIL's number; the same tables as resample_coefficients for the first two."""
    lib = load_library()
    code = RESAMPLE_FILTERS_EX[filter] if isinstance(filter, str) else int(filter)
    ks = C.c_int32()
    if lib.pd_resample_coefficients_ex(int(in_size), int(out_size), code, C.byref(ks), None, None):
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    bounds = np.zeros((int(out_size), 2), np.int32)
    kk = np.zeros((int(out_size), ks.value), np.int32)
    if lib.pd_resample_coefficients_ex(int(in_size), int(out_size), code, C.byref(ks), bounds.ctypes.data, kk.ctypes.data):
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    return bounds, kk


def clip_preprocess_geometry(H: int, W: int, image_size: int = 224) -> Tuple[int, int, int, int]:
    """(Hr, Wr, top, left) of CLIPImageProcessor's shortest-edge resize and centre crop (pd_clip_preprocess_geometry; host only)."""
    lib = load_library()
    v = [C.c_int32() for _ in range(4)]
    if lib.pd_clip_preprocess_geometry(int(H), int(W), int(image_size), *[C.byref(x) for x in v]):
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    return tuple(int(x.value) for x in v)


def clip_patch_width(patch: int) -> int:
    """Row width of the patch GEMM's operand: 3 patch^2 rounded up to 8 (pd_clip_patch_width)."""
    return int(load_library().pd_clip_patch_width(int(patch)))


def clip_preprocess_supported(H: int, W: int, image_size: int = 224) -> bool:
    """Whether pd_clip_preprocess takes H x W pictures (no axis reduced beyond PD_RESAMPLE_MAX_SCALE); else keep the host processor."""
    Hr, Wr, _, _ = clip_preprocess_geometry(H, W, image_size)
    return resample_supported((H, W), (Hr, Wr))


def resample_supported(src_hw, dst_hw) -> bool:
    """Whether pd_image_load resamples src_hw = (Hs, Ws) to dst_hw = (H, W): no axis reduced beyond PD_RESAMPLE_MAX_SCALE."""
    return all(int(i) >= 1 and int(o) >= 1 and int(i) <= PD_RESAMPLE_MAX_SCALE * int(o) for i, o in zip(src_hw, dst_hw))


def make_config(cfg: ModelConfig, precision: int = PD_PREC_F16, stream_f32: bool = False) -> pd_config:
    c = pd_config()
    c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
    c.hint_channels, c.query_channels = cfg.hint_channels, cfg.query_channels
    c.model_channels = cfg.model_channels
    c.num_levels = len(cfg.channel_mult)
    for i, m in enumerate(cfg.channel_mult):
        c.channel_mult[i] = m
    c.num_res_blocks = cfg.num_res_blocks
    c.num_attn_res = len(cfg.attention_resolutions)
    for i, m in enumerate(cfg.attention_resolutions):
        c.attention_resolutions[i] = m
    c.num_heads = cfg.num_heads
    c.context_dim, c.context_len = cfg.context_dim, cfg.context_len
    for i, m in enumerate(cfg.hint_widths):
        c.hint_widths[i] = m
    c.timesteps = cfg.timesteps
    c.linear_start, c.linear_end = cfg.linear_start, cfg.linear_end
    c.precision = precision
    c.stream_f32 = 1 if stream_f32 else 0
    c.vae_ch = cfg.vae_ch
    c.vae_num_levels = len(cfg.vae_ch_mult)
    for i, m in enumerate(cfg.vae_ch_mult):
        c.vae_ch_mult[i] = m
    c.vae_num_res_blocks, c.vae_out_ch, c.scale_factor = cfg.vae_num_res_blocks, cfg.vae_out_ch, cfg.scale_factor
    c.text_vocab, c.text_layers, c.text_heads, c.text_ff = cfg.text_vocab, cfg.text_layers, cfg.text_heads, cfg.text_ff
    c.vae_encoder = 1 if cfg.vae_encoder else 0
    return c


def alphas_cumprod(cfg: ModelConfig) -> np.ndarray:
    """The engine's noise schedule in fp64: make_beta_schedule('linear') (betas linear in sqrt space), cumulative product
    of 1 - beta -- the values the fused UniPC coefficients are derived from (pd_unipc_coefficients)."""
    T = cfg.timesteps
    s0, s1 = np.sqrt(cfg.linear_start), np.sqrt(cfg.linear_end)
    st = (s1 - s0) / (T - 1) if T > 1 else 0.0
    b = s0 + st * np.arange(T, dtype=np.float64)
    b[-1] = s1
    return np.cumprod(1.0 - b * b)


def _unipc_args(order: int, solver_type: str, lower_order_final: bool, disable_corrector) -> Tuple[pd_unipc_args, np.ndarray]:
    if solver_type not in ("bh1", "bh2"):
        raise ValueError("solver_type must be 'bh1' or 'bh2'")
    dc = np.ascontiguousarray(np.asarray(list(disable_corrector), dtype=np.int64).astype(np.int32).reshape(-1))
    u = pd_unipc_args()
    u.order, u.bh2, u.lower_order_final = int(order), 1 if solver_type == "bh2" else 0, 1 if lower_order_final else 0
    u.n_disable_corrector = len(dc)
    u.disable_corrector = dc.ctypes.data if len(dc) else None
    return u, dc


def unipc_coefficients(cfg: ModelConfig, timesteps, order: int = 2, solver_type: str = "bh2", lower_order_final: bool = True,
                       disable_corrector: Sequence[int] = ()) -> np.ndarray:
    """Per-step coefficient rows [steps, PD_UNIPC_NCOEF] (fp64) of the fused UniPC loop for the grid `timesteps` (sampling
    order); row layout in include/pdengine.h.  Host only: needs the library, not a GPU."""
    lib = load_library()
    ts = np.ascontiguousarray(_to_host(timesteps), dtype=np.int64).reshape(-1)
    u, dc = _unipc_args(order, solver_type, lower_order_final, disable_corrector)
    c = make_config(cfg)
    out = np.zeros((max(len(ts), 1), PD_UNIPC_NCOEF), np.float64)
    if lib.pd_unipc_coefficients(C.byref(c), C.byref(u), ts.ctypes.data if len(ts) else None, len(ts), out.ctypes.data) != 0:
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    del dc
    return out[:len(ts)]


def _lms_args(kind: str, order: int, solver_type: str, lower_order_final: bool, model_times=None, rows=None, row_times=None):
    """pd_lms_args and the arrays it points to (keep them alive for the call)."""
    if kind not in _LMS_KINDS:
        raise ValueError(f"kind must be one of {sorted(_LMS_KINDS)}")
    if solver_type not in _LMS_SOLVER_TYPES:
        raise ValueError(f"solver_type must be one of {sorted(_LMS_SOLVER_TYPES)}")
    u = pd_lms_args()
    u.kind, u.order = _LMS_KINDS[kind], int(order)
    u.solver_type, u.lower_order_final = _LMS_SOLVER_TYPES[solver_type], 1 if lower_order_final else 0
    keep = []
    if model_times is not None:
        mt = np.ascontiguousarray(_to_host(model_times), dtype=np.float64).reshape(-1)
        u.model_times = mt.ctypes.data
        keep.append(mt)
    if kind == "rows":
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, PD_LMS_NCOEF)
        rt = np.ascontiguousarray(row_times, dtype=np.float64).reshape(-1)
        if len(r) != len(rt):
            raise ValueError("rows and row_times must have one entry per evaluation")
        u.rows, u.row_times, u.n_rows = r.ctypes.data, rt.ctypes.data, len(rt)
        keep += [r, rt]
    return u, keep


def _lms_steps(timesteps, model_times, steps) -> int:
    if model_times is not None:
        return len(np.asarray(_to_host(model_times)).reshape(-1)) - 1
    if timesteps is not None:
        return len(np.asarray(_to_host(timesteps)).reshape(-1))
    if steps is None:
        raise ValueError("a linear multistep loop needs timesteps, model_times or (with its own rows) steps")
    return int(steps)


def lms_coefficients(cfg: ModelConfig, timesteps=None, kind: str = "dpmsolver++", order: int = 2, solver_type: str = "dpm_solver",
                     lower_order_final: bool = True, model_times=None, rows=None, row_times=None, steps: Optional[int] = None):
    """(rows [n_rows, PD_LMS_NCOEF], row_times [n_rows]) in fp64 of a linear multistep loop: `kind` "plms" or "dpmsolver++" over
    the grid `timesteps` (sampling order; lands on sigma = 0 for dpmsolver++), or dpmsolver++ over `model_times` (steps + 1
    possibly fractional times, the last one the landing point).  Row layout in include/pdengine.h.  Host only: needs the
    library, not a GPU."""
    lib = load_library()
    n = _lms_steps(timesteps, model_times, steps)
    ts = None if timesteps is None else np.ascontiguousarray(_to_host(timesteps), dtype=np.int64).reshape(-1)
    u, keep = _lms_args(kind, order, solver_type, lower_order_final, model_times, rows, row_times)
    c = make_config(cfg)
    if u.n_rows > n + 1:
        raise PdError(f"lms: {u.n_rows} rows do not fit the steps + 1 = {n + 1} that pd_lms_coefficients returns")
    cap = n + 1
    out = np.zeros((cap, PD_LMS_NCOEF), np.float64)
    times = np.zeros(cap, np.float64)
    nr = C.c_int32(0)
    if lib.pd_lms_coefficients(C.byref(c), C.byref(u), ts.ctypes.data if ts is not None and len(ts) else None, n, out.ctypes.data,
                               times.ctypes.data, C.byref(nr)) != 0:
        raise PdError(lib.pd_last_error().decode(errors="replace"))
    del keep
    return out[:nr.value], times[:nr.value]


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _to_host(x):
    return x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)


class _Buf:
    """A float32 (or int64) contiguous buffer as (pointer, mem-space), keeping its owner alive."""

    def __init__(self, x, dtype=np.float32):
        if x is None:
            self.owner, self.ptr, self.mem = None, None, None
            return
        if _is_torch(x):
            import torch
            td = torch.float32 if dtype == np.float32 else torch.int64
            t = x.detach().to(td).contiguous()
            self.owner, self.ptr = t, t.data_ptr()
            self.mem = PD_MEM_DEVICE if t.is_cuda else PD_MEM_HOST
        else:
            a = np.ascontiguousarray(x, dtype=dtype)
            self.owner, self.ptr, self.mem = a, a.ctypes.data, PD_MEM_HOST

    @property
    def device(self):
        """The torch device of a CUDA buffer, None for host memory (and for no buffer)."""
        return self.owner.device if self.mem == PD_MEM_DEVICE else None


def _new_out(shape, dtype=np.float32, device=None):
    """(output, pointer) of an uninitialised result: a torch tensor on `device` -- what a _Buf's .device gives for a CUDA caller --
    or, with device None, a NumPy array.  dtype: a NumPy type, or a torch dtype NumPy has no name for."""
    if device is None:
        out = np.empty(shape, dtype)
        return out, out.ctypes.data
    import torch
    out = torch.empty(shape, dtype=dtype if isinstance(dtype, torch.dtype) else getattr(torch, np.dtype(dtype).name), device=device)
    return out, out.data_ptr()


class Engine:
    """One engine <-> one GPU <-> one HIP stream (SURVEY.md §8b threading row)."""

    def __init__(self, cfg: ModelConfig = SD15, device: int = 0, precision: str = "f16", stream_f32: bool = False,
                 lib_path: Optional[str] = None):
        """precision: "f16" (default: the reference's own GPU dtype, README.md:44-45), "bf16", "f16x2" (split fp16
        operands over fp32 storage) or "f32"."""
        _torch_runtime_first()
        self.lib = load_library(lib_path)
        self.cfg = cfg
        self.precision = PRECISIONS[precision]
        self.device = device
        self._h = C.c_void_p()
        c = make_config(cfg, self.precision, stream_f32)
        self._check(self.lib.pd_engine_create(C.byref(c), device, C.byref(self._h)))
        if getattr(cfg, "hed", False):
            self._check(self.lib.pd_hed_configure(self._h))
        if getattr(cfg, "mlsd", False):
            self._check(self.lib.pd_mlsd_configure(self._h))
        self._clip_vision: Dict[str, ClipVisionConfig] = {}
        for cv in getattr(cfg, "clip_vision", ()) or ():
            self.configure_clip_vision(cv)
        if getattr(cfg, "safety_checker", False):
            self.configure_safety_checker()
        self._ip_adapter: Optional[Tuple[int, int]] = None    # (num_tokens, embed_dim) once configured
        if getattr(cfg, "ip_adapter", ()):
            self.configure_ip_adapter(*cfg.ip_adapter)
        self._keep: List[_Buf] = []
        self._rng_set = False    # the caller has chosen a seed (set_rng): draws nobody supplied may come from the engine

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise PdError(self.lib.pd_last_error().decode(errors="replace"))

    def _order_after_torch(self, mem: int, device=None) -> None:
        """CUDA tensors were produced on torch's current stream; the engine reads them on its own non-blocking streams.
        Make those wait for everything enqueued on the producer stream so far (incl. the .to()/.contiguous() copies _Buf
        just launched)."""
        if mem != PD_MEM_DEVICE:
            return
        import torch
        st = torch.cuda.current_stream(device)
        self._check(self.lib.pd_wait_stream(self._h, C.c_void_p(st.cuda_stream)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.pd_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def param_names(self) -> List[Tuple[str, Tuple[int, ...]]]:
        out = []
        name, nd, shp = C.c_char_p(), C.c_int32(), (C.c_int64 * 4)()
        for i in range(self.lib.pd_param_count(self._h)):
            self._check(self.lib.pd_param_info(self._h, i, C.byref(name), C.byref(nd), shp))
            out.append((name.value.decode(), tuple(int(shp[k]) for k in range(nd.value))))
        return out

    def load_tensor(self, name: str, array) -> None:
        if _is_torch(array):
            array = array.detach().float().cpu().numpy()
        a = np.ascontiguousarray(array)
        if a.dtype == np.float16:
            dt = PD_DT_F16
        else:
            a = a.astype(np.float32, copy=False)
            dt = PD_DT_F32
        shp = (C.c_int64 * max(1, a.ndim))(*a.shape)
        self._check(self.lib.pd_load_weights(self._h, name.encode(), a.ctypes.data, shp, a.ndim, dt))

    def load_state_dict(self, items: Iterable[Tuple[str, np.ndarray]], strict: bool = True) -> None:
        """Walk a reference checkpoint (``model.diffusion_model.*`` / ``control_model.*`` keys,
        cldm/model.py:12-21); ``first_stage_model.*`` / ``cond_stage_model.*`` tensors load into the parts this engine built
        (decoder, text transformer, and the encoder with ``vae_encoder=True``), everything else is skipped."""
        known = {n for n, _ in self.param_names()}
        it = items.items() if isinstance(items, dict) else items
        for name, arr in it:
            if name in known:
                self.load_tensor(name, arr)
        if strict and self.weights_missing():
            raise PdError(f"{self.weights_missing()} tensors missing after load_state_dict")

    def read_weight(self, name: str) -> np.ndarray:
        """One tensor back in its checkpoint layout as float32 (pd_read_weights): what the engine computes with, adapters
        merged."""
        shapes = getattr(self, "_shapes", None)
        if shapes is None:
            shapes = self._shapes = dict(self.param_names())
        if name not in shapes:
            raise PdError(f"pd_read_weights: unknown tensor '{name}'")
        out = np.empty(shapes[name], np.float32)
        self._check(self.lib.pd_read_weights(self._h, name.encode(), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ LoRA (pd_lora_*)
    def lora_add(self, adapter: int, name: str, up, down, alpha: Optional[float] = None) -> None:
        """Register one LoRA factor pair of adapter id `adapter` on tensor `name`: up [N, r] (or [N, r, 1, 1]), down [r, K] or
        [r, cin, kh, kw].  With `alpha`, up is multiplied by alpha / r first (in float32).  The adapter stays inactive until
        lora_set_scales gives it a non-zero scale."""
        up = np.asarray(_to_host(up), np.float32)
        down = np.ascontiguousarray(np.asarray(_to_host(down), np.float32))
        if up.ndim == 4 and up.shape[2:] == (1, 1):
            up = up[:, :, 0, 0]
        if up.ndim != 2:
            raise PdError(f"pd_lora_add: '{name}': up must be [N, r] or [N, r, 1, 1], got {up.shape}")
        r = up.shape[1]
        if alpha is not None:
            up = up * np.float32(float(alpha) / r)
        up = np.ascontiguousarray(up)
        shp = (C.c_int64 * max(1, down.ndim))(*down.shape)
        self._check(self.lib.pd_lora_add(self._h, int(adapter), name.encode(), up.ctypes.data, up.shape[0], r, down.ctypes.data,
                                         shp, down.ndim))

    def lora_add_ex(self, adapter: int, name: str, kind: str, up, down, up2=None, down2=None, scale: float = 1.0,
                    magnitude=None) -> None:
        """Register one adapter factor set that is not (only) a plain pair (pd_lora_add_ex).  With N, K = cin * kh * kw the
        tensor's rows and columns, the delta D is, by `kind`:
          "pair": scale * up @ down                         up [N, r], down [r, K] or [r, cin, kh, kw]
          "hada": scale * (up @ down) * (up2 @ down2)       (LoHa: w1_a, w1_b, w2_a, w2_b)
          "kron": scale * kron(up, down)                    up = w1 [a, b], down = w2 [c, d] or [c, d, kh, kw]; a c = N, b d = cin
        and `magnitude` [N] (DoRA) turns the contribution into (m / |W0 + s D|_row) (W0 + s D) - W0."""
        if kind not in LORA_KINDS:
            raise PdError(f"pd_lora_add_ex: '{name}': kind must be one of {sorted(LORA_KINDS)}, got {kind!r}")
        shapes = getattr(self, "_shapes", None)
        if shapes is None:
            shapes = self._shapes = dict(self.param_names())
        if name not in shapes:
            raise PdError(f"pd_lora_add_ex: unknown tensor '{name}'")
        shp = tuple(shapes[name])
        if len(shp) < 2:
            raise PdError(f"pd_lora_add_ex: '{name}' is a vector parameter (bias / norm); adapters apply to matrices")
        N, cin, tail = shp[0], shp[1], tuple(shp[2:])
        K = int(np.prod(shp[1:]))
        arr = lambda a: np.ascontiguousarray(np.asarray(_to_host(a), np.float32))
        f = LoraFactors(kind=LORA_KINDS[kind], scale=float(scale))
        keep = []

        def pair(u, d, what):
            u, d = arr(u), arr(d)
            if u.ndim == 4 and u.shape[2:] == (1, 1):
                u = np.ascontiguousarray(u[:, :, 0, 0])
            ok = u.ndim == 2 and u.shape[0] == N and d.ndim in (2, 4) and d.shape[0] == u.shape[1] and d.size == u.shape[1] * K
            if ok and d.ndim == 4:
                ok = d.shape[1] == cin and (not tail or tuple(d.shape[2:]) == tail)
            if not ok or u.shape[1] == 0:
                raise PdError(f"pd_lora_add_ex: '{name}': {what} {u.shape} / {d.shape} are not [{N}, r] and [r, {K}] (or [r, {cin}, kh, kw])")
            keep.extend((u, d))
            return u, d

        if kind == "kron":
            w1, w2 = arr(up), arr(down)
            taps = int(np.prod(tail)) if tail else 1
            if w2.ndim == 2 and taps > 1 and w2.shape[1] % taps == 0:   # a decomposed w2: [c, d * kh * kw]
                w2 = w2.reshape(w2.shape[0], -1, *tail)
            ok = w1.ndim == 2 and w2.ndim in (2, 4)
            if ok and w2.ndim == 4:
                ok = (tuple(w2.shape[2:]) == tail) if tail else w2.shape[2:] == (1, 1)
            if ok and w2.ndim == 2 and tail:
                ok = int(np.prod(tail)) == 1
            if not ok or w1.shape[0] * w2.shape[0] != N or w1.shape[1] * w2.shape[1] != cin:
                raise PdError(f"pd_lora_add_ex: '{name}': w1 {w1.shape} / w2 {w2.shape} do not satisfy a * c = {N} and b * d = {cin} "
                              f"with the kernel size {tail or (1, 1)}")
            keep.extend((w1, w2))
            f.kron_a, f.kron_b = w1.shape
            f.up, f.down = w1.ctypes.data, w2.ctypes.data
        else:
            u, d = pair(up, down, "up / down")
            f.rank, f.up, f.down = u.shape[1], u.ctypes.data, d.ctypes.data
            if kind == "hada":
                if up2 is None or down2 is None:
                    raise PdError(f"pd_lora_add_ex: '{name}': a Hadamard adapter needs up2 / down2")
                u2, d2 = pair(up2, down2, "up2 / down2")
                f.rank2, f.up2, f.down2 = u2.shape[1], u2.ctypes.data, d2.ctypes.data
        if magnitude is not None:
            m = arr(magnitude).reshape(-1)
            if m.size != N:
                raise PdError(f"pd_lora_add_ex: '{name}': the magnitude has {m.size} elements, the parameter has {N} rows")
            keep.append(m)
            f.magnitude = m.ctypes.data
        self._check(self.lib.pd_lora_add_ex(self._h, int(adapter), name.encode(), C.byref(f)))

    def lora_set_scales(self, scales: Sequence[float]) -> None:
        """Scale of adapter id i = scales[i] (0: inactive; ids past the end: 0); merges what changed on the device."""
        a = np.ascontiguousarray(np.asarray(list(scales), np.float32).reshape(-1))
        self._check(self.lib.pd_lora_set_scales(self._h, a.ctypes.data if a.size else None, a.size))

    def lora_remove(self, adapter: int = -1) -> None:
        """Forget adapter id `adapter` (-1: all); tensors no adapter touches get their base weights back bit-exactly."""
        self._check(self.lib.pd_lora_remove(self._h, int(adapter)))

    # ------------------------------------------------------------------ FreeU (pd_set_freeu)
    def set_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """FreeU (arXiv:2309.11497) in every later UNet evaluation of this engine, as diffusers' unet.enable_freeu: the first
        two decoder stages scale half their backbone channels by b1 / b2 and the lowest frequencies of their skip tensors by
        s1 / s2.  Any value 0 leaves the UNet exactly as without FreeU; non-finite values raise PdError."""
        self._check(self.lib.pd_set_freeu(self._h, float(s1), float(s2), float(b1), float(b2)))

    def disable_freeu(self) -> None:
        self._check(self.lib.pd_set_freeu(self._h, 0.0, 0.0, 0.0, 0.0))

    @property
    def freeu(self) -> Optional[Tuple[float, float, float, float]]:
        """(s1, s2, b1, b2) as last set (as float32), or None after disable_freeu / before any set_freeu."""
        out = (C.c_float * 4)()
        self._check(self.lib.pd_get_freeu(self._h, out))
        v = tuple(float(x) for x in out)
        return None if not any(v) else v

    # ------------------------------------------------------------------ perturbed-attention guidance (pd_set_pag)
    def set_pag(self, scale: float, layers, adaptive_scale: float = 0.0) -> None:
        """Perturbed-attention guidance (arXiv:2403.17377, as diffusers' PAGMixin) in every later guided evaluation of this engine: a
        third branch, the conditional one with the self-attention of the UNet transformer blocks in `layers` replaced by the identity,
        and eps += p_i (eps_cond - eps_perturbed), p_i = scale, or max(scale - adaptive_scale (1000 - t_i), 0).  `layers` is a bit
        mask or an iterable of block indices (encoder blocks, then decoder blocks, then the middle block: parse_pag_layers of
        prompt_diffusion_amd.pag turns diffusers' names into one).  Scale 0 or no layer leaves every call exactly as without it;
        negative or non-finite values and blocks the UNet does not have raise PdError."""
        if isinstance(layers, (int, np.integer)):
            mask = int(layers)
        else:
            mask = 0
            for j in layers:
                if not 0 <= int(j) < 32:
                    raise ValueError(f"set_pag: block index {j} outside 0 .. 31")
                mask |= 1 << int(j)
        if not 0 <= mask < 2 ** 32:
            raise ValueError(f"set_pag: layer mask {mask:#x} does not fit 32 bits")
        self._check(self.lib.pd_set_pag(self._h, float(scale), float(adaptive_scale), mask))

    def disable_pag(self) -> None:
        self._check(self.lib.pd_set_pag(self._h, 0.0, 0.0, 0))

    @property
    def pag(self) -> Optional[Tuple[float, float, int]]:
        """(scale, adaptive_scale, layer mask) as last set (the scales as float32), or None while it is off (scale 0 or mask 0)."""
        out, mask = (C.c_float * 2)(), C.c_uint32(0)
        self._check(self.lib.pd_get_pag(self._h, out, C.byref(mask)))
        if float(out[0]) == 0.0 or mask.value == 0:
            return None
        return float(out[0]), float(out[1]), int(mask.value)

    # ------------------------------------------------------------------ seeded noise (pd_set_rng / pd_randn)
    def set_rng(self, seed: int, sample_base: int = 0) -> None:
        """Seed of the engine's Philox generator and the global index of this engine's first sample: the draw of sample b is
        that of sample `sample_base + b` of an unsharded run.  Takes effect for everything enqueued afterwards, captured
        graphs included (they are kept)."""
        self._check(self.lib.pd_set_rng(self._h, int(seed) & (2 ** 64 - 1), int(sample_base) & (2 ** 64 - 1)))
        self._rng_set = True

    @property
    def rng(self) -> Tuple[int, int]:
        """(seed, sample_base) as last set; (0, 0) on a new engine."""
        s, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.pd_get_rng(self._h, C.byref(s), C.byref(b)))
        return int(s.value), int(b.value)

    def randn(self, shape, stream="step", draw: int = 0, device=None):
        """The standard normals the engine draws at (stream, draw) for shape[0] samples of prod(shape[1:]) elements each (NCHW
        order within a sample): stream "xt" (the start latents), "step" (draw = step / row index), "vae" (the posterior
        sample) or an int (PD_RNG_USER + k for draws of the caller's own).  NumPy, or a CUDA tensor with device=."""
        st = RNG_STREAMS[stream] if isinstance(stream, str) else int(stream)
        shape = tuple(int(v) for v in shape)
        B, per = shape[0], int(np.prod(shape[1:], dtype=np.int64))
        out, op = _new_out(shape, device=device)
        self._check(self.lib.pd_randn(self._h, st, int(draw), B, per, PD_MEM_HOST if device is None else PD_MEM_DEVICE, op))
        return out

    def init_random_weights(self, seed: int = 1234) -> None:
        self._check(self.lib.pd_init_random_weights(self._h, seed))

    def weights_missing(self) -> int:
        return int(self.lib.pd_weights_missing(self._h))

    def vae_weights_missing(self) -> int:
        return int(self.lib.pd_vae_weights_missing(self._h))

    def vae_decode(self, latents):
        """decode_first_stage (ddpm.py:820-828): latents [B,4,h,w] -> images [B,3,8h,8w] in about [-1, 1]."""
        b = _Buf(latents)
        B, _, h, w = b.owner.shape
        out, op = _new_out((B, self.cfg.vae_out_ch, 8 * h, 8 * w), device=b.device)
        self._order_after_torch(b.mem)
        self._check(self.lib.pd_vae_decode(self._h, b.ptr, B, h, w, b.mem, op))
        return out

    def vae_encoder_weights_missing(self) -> int:
        return int(self.lib.pd_vae_encoder_weights_missing(self._h))

    # ------------------------------------------------------------------ tiled / sliced VAE calls (pd_vae_set_tiling)
    _vae_which = PD_VAE_SD15

    def set_vae_tiling(self, on: bool = True, tile_latent: Optional[int] = None, overlap_factor: Optional[float] = None,
                       tile_batch: Optional[int] = None) -> None:
        """diffusers' vae.enable_tiling / disable_tiling for every later vae_decode / vae_encode of this engine: a latent larger than
        tile_latent (an image larger than 8 * tile_latent) per side is cut into overlapping tiles that run through the VAE on their own
        and are blended over overlap_factor of a tile; smaller calls run exactly as without.  With on=True the three parameters replace
        what was set, None: the default (64 latent pixels, 0.25, 4 tiles per batch); with on=False a None keeps what was set.  The result
        is diffusers' tiled one, not the untiled image."""
        self._check(self.lib.pd_vae_set_tiling(self._h, self._vae_which, int(bool(on)), int(tile_latent or 0), float(overlap_factor or 0.0),
                                               int(tile_batch or 0)))

    def set_vae_slicing(self, on: bool = True) -> None:
        """diffusers' vae.enable_slicing / disable_slicing: with more than one sample, each is decoded / encoded on its own."""
        self._check(self.lib.pd_vae_set_slicing(self._h, self._vae_which, int(bool(on))))

    @property
    def vae_tiling(self) -> VaeTilingState:
        """(tiling, slicing, tile_latent, overlap_factor, tile_batch) with the defaults resolved."""
        t, s, n, b, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.pd_vae_get_tiling(self._h, self._vae_which, C.byref(t), C.byref(s), C.byref(n), C.byref(f), C.byref(b)))
        return VaeTilingState(bool(t.value), bool(s.value), int(n.value), float(f.value), int(b.value))

    def vae_tile_plan(self, h: int, w: int, encode: bool = False) -> VaeTilePlan:
        """The grid a vae_decode of an h x w latent (encode=True: a vae_encode of an h x w image) takes with the tiling parameters as
        set, whether or not tiling is switched on; rows = cols = 0 where the size is not tiled."""
        st = self.vae_tiling
        return vae_tile_plan(h, w, st.tile_latent, st.overlap_factor, 8, encode)

    def op_vae_tile_blend(self, tiles, plan: VaeTilePlan, C_out: int, nchw: bool = True):
        """vae_tile_blend_kernel alone (pd_op_vae_tile_blend): tiles = one fp32 array [B, th, tw, Cpad] per tile of the plan, row-major;
        -> [B, C_out, H, W] (nchw) or [B, H, W, Cpad]."""
        n = plan.rows * plan.cols
        buf = (pd_vae_tile * n)()
        for i, t in enumerate(plan.tiles):
            for f in VaeTile._fields:
                setattr(buf[i], f, int(getattr(t, f)))
        B, cpad = int(tiles[0].shape[0]), int(tiles[0].shape[3])
        flat = np.concatenate([np.ascontiguousarray(t, np.float32).reshape(-1) for t in tiles])
        last = plan.tiles[-1]
        H, Wd = last.oy + last.oh, last.ox + last.ow
        out = np.empty((B, C_out, H, Wd) if nchw else (B, H, Wd, cpad), np.float32)
        self._check(self.lib.pd_op_vae_tile_blend(self._h, flat.ctypes.data, C.addressof(buf), plan.rows, plan.cols, B, int(C_out), cpad,
                                                  int(bool(nchw)), out.ctypes.data))
        return out

    def vae_encode(self, images, mode: str = "mean", noise=None):
        """AutoencoderKL.encode (autoencoder.py:83-87) on the device: images [B,3,H,W] in [-1, 1] (H, W multiples of 8,
        (H/8)*(W/8) a multiple of 64) ->
          "mean":    scale_factor * posterior.mode()                        [B,4,H/8,W/8]
          "sample":  scale_factor * (mean + std * noise), noise [B,4,H/8,W/8] standard normal from the caller, or drawn
                     by the engine (randn(..., "vae")) with noise="engine" -- also with noise=None once set_rng has been called
          "moments": quant_conv output (mean ; logvar), unscaled, unclamped  [B,8,H/8,W/8]
        NumPy in, NumPy out; CUDA tensors in (images and noise), CUDA tensor out."""
        if mode not in VAE_ENCODE_MODES:
            raise ValueError(f"mode must be one of {sorted(VAE_ENCODE_MODES)}")
        what = VAE_ENCODE_MODES[mode]
        if isinstance(noise, str):
            if noise != "engine":
                raise ValueError("noise must be an array or \"engine\"")
            noise = None
        elif noise is None and what == PD_VAE_SAMPLE and not self._rng_set:
            raise PdError("pd_vae_encode: PD_VAE_SAMPLE needs `noise` [B, z, H/8, W/8] (or noise=\"engine\" / Engine.set_rng "
                          "for the engine's own seeded draw)")
        b = _Buf(images)
        nb = _Buf(noise)
        if nb.mem is not None and nb.mem != b.mem:
            raise PdError("images and noise must live in the same memory space")
        B, _, H, W = b.owner.shape
        z = self.cfg.in_channels
        out, op = _new_out((B, 2 * z if what == PD_VAE_MOMENTS else z, H // 8, W // 8), device=b.device)
        if nb.owner is not None and tuple(nb.owner.shape) != (B, z, H // 8, W // 8):
            raise ValueError(f"noise must be [{B}, {z}, {H // 8}, {W // 8}]")
        self._order_after_torch(b.mem)
        self._check(self.lib.pd_vae_encode(self._h, b.ptr, B, H, W, b.mem, what, nb.ptr if what == PD_VAE_SAMPLE else None, op))
        return out

    # ------------------------------------------------------------------ HED edge detector (pd_hed_*)
    def hed_weights_missing(self) -> int:
        return int(self.lib.pd_hed_weights_missing(self._h))

    def load_hed_state_dict(self, sd) -> None:
        """Load the HED ``Network``'s 38 tensors from the checkpoint's ``module...`` keys (network-bsds500.pth), ``Network``'s own
        ``net...`` keys or the registry's ``hed.net...`` names; an unknown key raises PdError."""
        it = sd.items() if isinstance(sd, dict) else sd
        for name, arr in it:
            try:
                key = hed_key(name)
            except KeyError as ex:
                raise PdError(f"load_hed_state_dict: {ex.args[0]}") from None
            self.load_tensor(key, arr)

    def hed(self, images, what: str = "edge"):
        """HED edge detection (annotator/hed/__init__.py: HEDdetector.__call__ + Network.forward) on the device: images
        [B,3,H,W] float32 RGB in [0, 1], H and W multiples of 16 ->
          "edge":  sigmoid(netCombine(...)) in [0, 1]                          [B,1,H,W]
          "sides": the five score maps, upsampled to H x W, before netCombine  [B,5,H,W]
        NumPy in, NumPy out; CUDA tensor in, CUDA tensor out.  Needs ModelConfig(hed=True) and the hed.* weights."""
        if what not in HED_OUTPUTS:
            raise ValueError(f"what must be one of {sorted(HED_OUTPUTS)}")
        b = _Buf(images)
        if b.owner.ndim != 4 or b.owner.shape[1] != 3:
            raise ValueError(f"images must be [B, 3, H, W], got {tuple(b.owner.shape)}")
        B, _, H, W = b.owner.shape
        out, op = _new_out((B, 5 if what == "sides" else 1, H, W), device=b.device)
        self._order_after_torch(b.mem)
        self._check(self.lib.pd_hed_detect(self._h, b.ptr, B, H, W, b.mem, HED_OUTPUTS[what], op))
        return out

    # ------------------------------------------------------------------ CLIP image tower and safety checker (pd_clip_*, pd_safety_*)
    def configure_clip_vision(self, cfg: ClipVisionConfig = CLIP_VIT_H14, prefix: Optional[str] = None) -> None:
        """Register one CLIPVisionModelWithProjection under `prefix` (default: cfg.prefix) -- "image_encoder." or
        "safety_checker.vision_model." in a diffusers checkpoint; at most two per engine; configuring a prefix again does nothing."""
        import dataclasses
        if prefix is not None and prefix != cfg.prefix:
            cfg = dataclasses.replace(cfg, prefix=prefix)
        if cfg.act not in CLIP_ACTS:
            raise ValueError(f"act must be one of {sorted(CLIP_ACTS)}")
        if len(cfg.prefix.encode()) > 63:
            raise ValueError("prefix longer than 63 bytes")
        c = pd_clip_vision_config()
        c.hidden, c.layers, c.heads, c.ff, c.patch, c.image_size, c.proj_dim = (int(v) for v in (
            cfg.hidden, cfg.layers, cfg.heads, cfg.ff, cfg.patch, cfg.image_size, cfg.proj_dim))
        c.act, c.eps, c.stream_f32 = CLIP_ACTS[cfg.act], float(cfg.eps), int(bool(cfg.stream_f32))
        c.mean = (C.c_float * 3)(*cfg.mean)
        c.std = (C.c_float * 3)(*cfg.std)
        c.prefix = cfg.prefix.encode()
        self._check(self.lib.pd_clip_vision_configure(self._h, C.byref(c)))
        self._clip_vision.setdefault(cfg.prefix, cfg)
        self._shapes = None

    def configure_safety_checker(self, cfg: ClipVisionConfig = CLIP_VIT_L14_SAFETY) -> None:
        """The safety tower (if not there yet) and StableDiffusionSafetyChecker's four buffers (pd_safety_configure)."""
        if SAFETY_PREFIX not in self._clip_vision:
            self.configure_clip_vision(cfg, SAFETY_PREFIX)
        self._check(self.lib.pd_safety_configure(self._h))
        self._shapes = None

    # ------------------------------------------------------------------ IP-Adapter (pd_ip_adapter_*)
    def configure_ip_adapter(self, num_tokens: int = 4, embed_dim: int = 1024) -> None:
        """Registers the adapter's tensors (image_proj.*, ip_adapter.{2j+1}.to_k_ip / to_v_ip for the UNet's cross-attention blocks j in
        diffusers' processor order) in a registry group of their own; they load through load_state_dict.  Once per engine; a second
        call with the same numbers does nothing."""
        if self._ip_adapter is not None:
            if self._ip_adapter != (int(num_tokens), int(embed_dim)):
                raise NotImplementedError(f"this engine's registry already holds an IP-Adapter with (num_tokens, embed_dim) = {self._ip_adapter}; "
                                          f"one with {(int(num_tokens), int(embed_dim))} needs a new engine (tensors cannot be re-registered)")
            return
        c = pd_ip_adapter_config(num_tokens=int(num_tokens), embed_dim=int(embed_dim))
        self._check(self.lib.pd_ip_adapter_configure(self._h, C.byref(c)))
        self._ip_adapter = (int(num_tokens), int(embed_dim))
        self._shapes = None

    @property
    def ip_adapter_blocks(self) -> int:
        """Cross-attention blocks of the UNet (16 for the SD1.5 topology): the length of a per-block scale list."""
        from .weights import decoder_layout, encoder_layout
        return sum(b["attn"] for b in encoder_layout(self.cfg)) + sum(b["attn"] for b in decoder_layout(self.cfg)) + 1

    def ip_adapter_weights_missing(self) -> int:
        return self.lib.pd_ip_adapter_weights_missing(self._h)

    def ip_adapter_set_scale(self, scale) -> None:
        """One scale for every block, or one per block (ip_adapter_blocks values, processor order).  0 everywhere switches the adapter
        off: the engine then launches exactly what it launches without one."""
        s = np.ascontiguousarray(np.atleast_1d(np.asarray(scale, np.float32)).reshape(-1))
        self._check(self.lib.pd_ip_adapter_set_scale(self._h, s.ctypes.data, int(s.size)))

    def ip_adapter_scale(self) -> np.ndarray:
        out = np.zeros(self.ip_adapter_blocks, np.float32)
        self._check(self.lib.pd_ip_adapter_get_scale(self._h, out.ctypes.data, int(out.size)))
        return out

    def ip_adapter_set_image(self, embeds, negative_embeds=None) -> None:
        """embeds [Bi, E] (NumPy or a CUDA tensor): the image embeddings of the conditional half; negative_embeds [Bi, E] or None (zeros).
        Runs the projection and every block's K / V GEMMs now; every later UNet evaluation of this engine adds the image term until
        ip_adapter_clear_image.  A sampling call of batch B needs Bi == B or Bi == 1."""
        c = _Buf(embeds)
        if c.owner.ndim != 2:
            raise ValueError(f"ip_adapter_set_image: embeds must be [Bi, E], got {tuple(c.owner.shape)}")
        n = None
        if negative_embeds is not None:
            n = _Buf(negative_embeds)
            if tuple(n.owner.shape) != tuple(c.owner.shape) or n.mem != c.mem:
                raise ValueError("ip_adapter_set_image: negative_embeds must match embeds in shape and memory space")
        if self._ip_adapter is not None and int(c.owner.shape[1]) != self._ip_adapter[1]:
            raise ValueError(f"ip_adapter_set_image: embeddings of width {int(c.owner.shape[1])}, the adapter takes {self._ip_adapter[1]}")
        self._order_after_torch(c.mem, c.device)
        self._check(self.lib.pd_ip_adapter_set_image(self._h, c.ptr, None if n is None else n.ptr, int(c.owner.shape[0]), c.mem))

    def ip_adapter_clear_image(self) -> None:
        self._check(self.lib.pd_ip_adapter_clear_image(self._h))

    def bench_ip_attention(self, B: int, N: int, Cc: int, T: int = 4, iters: int = 50) -> Tuple[float, float]:
        """(ms per launch of the image term's kernel, ms per device-to-device copy of the 3 B N C elements it moves), random data"""
        k, c = C.c_float(), C.c_float()
        self._check(self.lib.pd_bench_ip_attention(self._h, B, N, Cc, T, iters, C.byref(k), C.byref(c)))
        return float(k.value), float(c.value)

    def _clip_prefix(self, prefix: Optional[str]) -> str:
        if prefix is None:
            if len(self._clip_vision) != 1:
                raise PdError("clip_vision: name the tower (prefix=...): this engine has " + (f"{len(self._clip_vision)}" if self._clip_vision else "none"))
            return next(iter(self._clip_vision))
        if prefix not in self._clip_vision:
            raise PdError(f"clip_vision: no image tower under '{prefix}' (configure_clip_vision)")
        return prefix

    def clip_vision_weights_missing(self, prefix: Optional[str] = None) -> int:
        return int(self.lib.pd_clip_vision_weights_missing(self._h, self._clip_prefix(prefix).encode()))

    def safety_weights_missing(self) -> int:
        return int(self.lib.pd_safety_weights_missing(self._h))

    def load_clip_vision_state_dict(self, sd, prefix: Optional[str] = None, strict: bool = True) -> None:
        """Load one tower (and, under the safety prefix, the checker's buffers) from a diffusers checkpoint's keys, or from the bare
        module's own: CLIPVisionModelWithProjection.state_dict() ("vision_model.*", "visual_projection.weight") and
        StableDiffusionSafetyChecker.state_dict() ("vision_model.vision_model.*", "visual_projection.weight", "concept_embeds", ...)
        are re-homed under the tower's prefix.  Keys the registry does not know (position_ids, other components) are skipped."""
        prefix = self._clip_prefix(prefix)
        cfg = self._clip_vision[prefix]
        known = set(clip_vision_param_shapes(cfg))
        if prefix == SAFETY_PREFIX:   # the checker's buffers travel with their tower, where pd_safety_configure registered them
            registered = {n for n, _ in self.param_names()}
            known |= {k for k in safety_param_shapes(cfg.proj_dim) if k in registered}
        outer = cfg.outer_prefix
        it = sd.items() if isinstance(sd, dict) else sd
        for name, arr in it:
            for cand in (name, outer + name, prefix + name):
                if cand in known:
                    self.load_tensor(cand, arr)
                    break
        if strict:
            n = self.clip_vision_weights_missing(prefix) + (self.safety_weights_missing() if prefix == SAFETY_PREFIX else 0)
            if n:
                raise PdError(f"{n} tensors missing after load_clip_vision_state_dict('{prefix}')")

    def clip_preprocess(self, images, image_size: int = 224, patch: int = 14, what: str = "pixel_values", mean=None, std=None,
                        host: bool = False):
        """CLIPImageProcessor() with its defaults on uint8 pictures [B, H, W, 3] (NumPy, or a CPU / CUDA torch tensor), on the device
        (pd_clip_preprocess): shortest edge to image_size with PIL BICUBIC, centre crop, (v / 255 - mean) / std in float32.
          "pixel_values": float32 [B, 3, S, S]
          "patches":      the patch GEMM's operand rows [B (S / patch)^2, round_up(3 patch^2, 8)] in the engine's operand type (float32,
                          or float16 / bfloat16 bit patterns as uint16 where NumPy comes out)
          "bytes":        uint8 [B, S, S, 3], the resized and cropped picture
        A CUDA tensor comes out; NumPy with host=True or for a NumPy input.  PdError for a reduction beyond PD_RESAMPLE_MAX_SCALE
        (clip_preprocess_supported): callers keep their host processor there."""
        if what not in CLIP_PREPROCESS_OUTPUTS:
            raise ValueError(f"what must be one of {sorted(CLIP_PREPROCESS_OUTPUTS)}")
        owner, sp, smem, sh = self._u8_source(images)
        if len(sh) != 4 or sh[3] != 3:
            raise ValueError(f"images must be uint8 [B, H, W, 3], got {tuple(sh)}")
        B, H, W, S = int(sh[0]), int(sh[1]), int(sh[2]), int(image_size)
        two_byte = self.precision in (PD_PREC_F16, PD_PREC_BF16)
        if what == "pixel_values":
            shape, ndt = (B, 3, S, S), np.float32
        elif what == "bytes":
            shape, ndt = (B, S, S, 3), np.uint8
        else:
            if S % int(patch):
                raise ValueError(f"image_size {S} is no multiple of patch {patch}")
            shape, ndt = (B * (S // int(patch)) ** 2, clip_patch_width(patch)), (np.uint16 if two_byte else np.float32)
        to_host = host or (smem == PD_MEM_HOST and not _is_torch(images))
        dmem = PD_MEM_HOST if to_host else PD_MEM_DEVICE
        if not to_host and ndt == np.uint16:   # the operand type itself on the device
            import torch
            ndt = torch.float16 if self.precision == PD_PREC_F16 else torch.bfloat16
        out, dp = _new_out(shape, ndt, None if to_host else self._torch_device())
        a = pd_clip_preprocess_args()
        a.src, a.B, a.H, a.W, a.mem_src = sp, B, H, W, smem
        a.image_size, a.patch, a.out_mode, a.mem_dst, a.dst = S, int(patch), CLIP_PREPROCESS_OUTPUTS[what], dmem, dp
        from .weights import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
        a.mean = (C.c_float * 3)(*(OPENAI_CLIP_MEAN if mean is None else mean))
        a.std = (C.c_float * 3)(*(OPENAI_CLIP_STD if std is None else std))
        self._order_after_torch(PD_MEM_DEVICE if PD_MEM_DEVICE in (smem, dmem) else PD_MEM_HOST)
        self._check(self.lib.pd_clip_preprocess(self._h, C.byref(a)))
        del owner
        return out

    def clip_vision(self, x, what="embeds", hidden_layer: int = -2, prefix: Optional[str] = None):
        """One forward pass of an image tower (pd_clip_vision_forward).  x: uint8 pictures [B, H, W, 3] (preprocessed on the device,
        straight into the patch matrix) or float32 pixel_values [B, 3, S, S]; NumPy or torch.  what: "embeds" (image_embeds [B, D]),
        "pooled" (pooler_output [B, C]), "hidden" (hidden_states[hidden_layer] [B, P + 1, C]; -2 is encode_image's), or a tuple of
        them (a tuple comes back).  NumPy in, NumPy out; CUDA tensor in, CUDA tensor out."""
        prefix = self._clip_prefix(prefix)
        cfg = self._clip_vision[prefix]
        names = (what,) if isinstance(what, str) else tuple(what)
        if not names or any(n not in CLIP_VISION_OUTPUTS for n in names):
            raise ValueError(f"what must be among {CLIP_VISION_OUTPUTS}")
        is_u8 = (x.dtype == np.uint8) if not _is_torch(x) else str(x.dtype) == "torch.uint8"
        if is_u8:
            owner, ptr, mem, sh = self._u8_source(x)
            if len(sh) != 4 or sh[3] != 3:
                raise ValueError(f"pictures must be uint8 [B, H, W, 3], got {tuple(sh)}")
            B, H, W = int(sh[0]), int(sh[1]), int(sh[2])
            dev = owner.device if mem == PD_MEM_DEVICE else None
        else:
            b = _Buf(x)
            owner, ptr, mem = b.owner, b.ptr, b.mem
            if owner.ndim != 4 or owner.shape[1] != 3:
                raise ValueError(f"pixel_values must be [B, 3, S, S], got {tuple(owner.shape)}")
            B, H, W = int(owner.shape[0]), int(owner.shape[2]), int(owner.shape[3])
            dev = owner.device if mem == PD_MEM_DEVICE else None
        shapes = {"embeds": (B, cfg.proj_dim), "pooled": (B, cfg.hidden), "hidden": (B, cfg.patches + 1, cfg.hidden)}
        made = {n: _new_out(shapes[n], device=dev) for n in names}
        outs = {n: o for n, (o, _) in made.items()}
        ptr_of = lambda n: made[n][1] if n in made else None
        a = pd_clip_vision_args()
        pre = prefix.encode()
        a.prefix, a.input, a.input_kind = pre, ptr, PD_CLIP_IN_U8 if is_u8 else PD_CLIP_IN_PIXEL_VALUES
        a.B, a.H, a.W, a.mem, a.hidden_layer = B, H, W, mem, int(hidden_layer)
        a.image_embeds, a.pooler_output, a.hidden = ptr_of("embeds"), ptr_of("pooled"), ptr_of("hidden")
        self._order_after_torch(mem)
        self._check(self.lib.pd_clip_vision_forward(self._h, C.byref(a)))
        del owner
        return outs[names[0]] if isinstance(what, str) else tuple(outs[n] for n in names)

    def safety_check(self, images_or_embeds, return_scores: bool = False):
        """StableDiffusionSafetyChecker.forward (pd_safety_check).  uint8 pictures [B, H, W, 3] go through the safety tower first;
        float32 [B, D] is taken as its image_embeds.  Returns the per-image flags as a bool array [B]; with return_scores also the
        float32 [B, 20] scores (3 special-care, then 17 concept, unrounded).  NumPy out (CUDA inputs are read on the device)."""
        x = images_or_embeds
        is_u8 = (x.dtype == np.uint8) if not _is_torch(x) else str(x.dtype) == "torch.uint8"
        if is_u8:
            x = self.clip_vision(x, "embeds", prefix=SAFETY_PREFIX)
        b = _Buf(x)
        if b.owner.ndim != 2:
            raise ValueError(f"embeds must be [B, D], got {tuple(b.owner.shape)}")
        B = int(b.owner.shape[0])
        flags, fp = _new_out((B,), np.int32, b.device)
        scores, sp = _new_out((B, PD_SAFETY_SPECIAL + PD_SAFETY_CONCEPTS), device=b.device) if return_scores else (None, None)
        self._order_after_torch(b.mem)
        self._check(self.lib.pd_safety_check(self._h, b.ptr, B, b.mem, fp, sp))
        flags = _to_host(flags).astype(bool)
        return (flags, _to_host(scores)) if return_scores else flags

    def safety_blank(self, images, flags, value: float = 0.0):
        """Write `value` over the flagged images of a CUDA float32 batch [B, ...] in place (pd_safety_blank) and return it.  0 is
        what the checker writes; with image_store(mul, add) behind it, -add / mul makes the stored picture black."""
        import torch
        if not (_is_torch(images) and images.is_cuda and images.dtype == torch.float32 and images.is_contiguous()):
            raise ValueError("images must be a contiguous float32 CUDA tensor")
        f = np.ascontiguousarray(np.asarray(_to_host(flags)).astype(np.int32))
        B = int(images.shape[0])
        if f.shape != (B,):
            raise ValueError(f"flags must be [{B}]")
        self._order_after_torch(PD_MEM_DEVICE)
        self._check(self.lib.pd_safety_blank(self._h, images.data_ptr(), B, int(images[0].numel()), f.ctypes.data, PD_MEM_HOST, float(value)))
        return images

    # ------------------------------------------------------------------ M-LSD line detector (pd_mlsd_*)
    def mlsd_weights_missing(self) -> int:
        return int(self.lib.pd_mlsd_weights_missing(self._h))

    def load_mlsd_state_dict(self, sd) -> None:
        """Load an M-LSD checkpoint (mlsd_large_512_fp32.pth) as it is: ``MobileV2_MLSD_Large.state_dict()`` keys, with or without the
        registry's ``mlsd.`` prefix -- conv weights (and biases), BatchNorm weight / bias / running_mean / running_var (eps 1e-5;
        num_batches_tracked is ignored).  Every BatchNorm is folded into the conv in front of it in float64, rounded once to float32
        (weights.fold_mlsd_state_dict), and one weight and one bias per conv are uploaded."""
        try:
            folded = fold_mlsd_state_dict(sd)
        except (KeyError, ValueError) as ex:
            raise PdError(f"load_mlsd_state_dict: {ex.args[0]}") from None
        for name, arr in folded.items():
            self.load_tensor(name, arr)

    def mlsd(self, images, thr_v: float = 0.1, thr_d: float = 0.1, what: str = "lines", *, out=None, c_off: int = 0, mul: float = 1.0,
             add: float = 0.0, host: bool = False):
        """M-LSD line detection (annotator/mlsd: MLSDdetector.__call__, pred_lines, MobileV2_MLSD_Large) on the device: uint8
        pictures [B, H, W, 3] RGB (NumPy, or a CPU / CUDA torch tensor), H and W multiples of 32 ->
          "lines":    the kept segments drawn white on black (cv2.line, thickness 1)    uint8 [B, H, W] of 0 / 255
          "segments": (int32 [B, 200, 4] of (x0, y0, x1, y1), best score first; int32 [B] counts)
          "tpmap":    the network output                                                float32 [B, 9, H/2, W/2]
        The constant-one fourth channel and x / 127.5 - 1 happen inside.  Every image of the batch is handled on its own, as the
        reference handles its one.  A CUDA tensor comes out; NumPy with host=True or for a NumPy input.  out ("lines" only): an existing
        contiguous float32 [B, Cf, H, W] whose channels c_off .. c_off + 2 also receive (lines / 255) * mul + add, as Engine.canny's.
        Needs ModelConfig(mlsd=True) and the mlsd.* weights."""
        if what not in MLSD_OUTPUTS:
            raise ValueError(f"what must be one of {sorted(MLSD_OUTPUTS)}")
        owner, sp, smem, sh = self._u8_source(images)
        if len(sh) != 4 or sh[3] != 3:
            raise ValueError(f"images must be uint8 [B, H, W, 3], got {tuple(sh)}")
        B, H, W = int(sh[0]), int(sh[1]), int(sh[2])
        a = pd_mlsd_args()
        a.images, a.B, a.H, a.W, a.mem, a.what = sp, B, H, W, smem, MLSD_OUTPUTS[what]
        a.thr_v, a.thr_d, a.mul, a.add = float(thr_v), float(thr_d), 1.0, 0.0
        if out is not None:
            if what != "lines":
                raise ValueError("out goes with what='lines'")
            if len(out.shape) != 4 or tuple(out.shape) != (B, out.shape[1], H, W):
                raise ValueError(f"out must be [{B}, Cf, {H}, {W}], got {tuple(out.shape)}")
            if _is_torch(out):
                import torch
                if out.dtype != torch.float32 or not out.is_contiguous():
                    raise ValueError("out must be a contiguous float32 tensor")
                a.dst_f, a.mem_f = out.data_ptr(), PD_MEM_DEVICE if out.is_cuda else PD_MEM_HOST
            else:
                if out.dtype != np.float32 or not out.flags.c_contiguous:
                    raise ValueError("out must be a C-contiguous float32 array")
                a.dst_f, a.mem_f = out.ctypes.data, PD_MEM_HOST
            a.Cf, a.c_off, a.mul, a.add = int(out.shape[1]), int(c_off), float(mul), float(add)
        # the C entry keeps `out` in the memory space of `images`: a host result for a CUDA input is copied down afterwards
        on_dev = smem == PD_MEM_DEVICE
        if what == "tpmap":
            shape, dt = (B, 9, H // 2, W // 2), np.float32
        elif what == "segments":
            shape, dt = (B * MLSD_TOPK * 4 + B,), np.int32
        else:
            shape, dt = (B, H, W), np.uint8
        res, a.out = _new_out(shape, dt, owner.device if on_dev else None)
        self._order_after_torch(PD_MEM_DEVICE if on_dev or (out is not None and a.mem_f == PD_MEM_DEVICE) else PD_MEM_HOST)
        self._check(self.lib.pd_mlsd_detect_ex(self._h, C.byref(a)))
        del owner
        if on_dev and host:
            res = res.cpu().numpy()
        elif not on_dev and not host and _is_torch(images):
            import torch
            res = torch.from_numpy(res).to(self._torch_device())
        if what == "segments":
            return res[:B * MLSD_TOPK * 4].reshape(B, MLSD_TOPK, 4), res[B * MLSD_TOPK * 4:]
        return res

    # ------------------------------------------------------------------ image ends (pd_image_load / pd_image_store)
    def _torch_device(self):
        import torch
        return torch.device("cuda", self.device)

    @staticmethod
    def _u8_source(x):
        """uint8 NumPy array or uint8 torch tensor -> (owner, pointer, mem, shape)"""
        if _is_torch(x):
            import torch
            if x.dtype != torch.uint8:
                raise ValueError(f"expected a uint8 tensor, got {x.dtype}")
            t = x.detach().contiguous()
            return t, t.data_ptr(), PD_MEM_DEVICE if t.is_cuda else PD_MEM_HOST, tuple(t.shape)
        a = np.asarray(x)
        if a.dtype != np.uint8:
            raise ValueError(f"expected a uint8 array, got {a.dtype}")
        a = np.ascontiguousarray(a)
        return a, a.ctypes.data, PD_MEM_HOST, a.shape

    def image_load(self, images, size=None, *, out=None, c_off: int = 0, channels: int = 3, batch: Optional[int] = None,
                   batch_mode: str = "repeat", mul: float = 1.0, add: float = 0.0, filter="lanczos", host: bool = False):
        """uint8 pictures [Bs, Hs, Ws, 3] (NumPy, or a CPU / CUDA torch tensor) -> float32 [B, channels, H, W], written into
        channels c_off .. c_off + 2 (pd_image_load): resampled to size = (H, W) exactly as PIL's Image.resize(filter) does
        when the sizes differ, then (u8 / 255) * mul + add in float32 -- (1, 0) for [0, 1], (2, -1) for [-1, 1].  batch: B, a
        multiple of Bs; batch_mode "repeat" reads source b // (B // Bs) (np.repeat), "tile" source b % Bs.  out: an existing
        contiguous float32 tensor (CUDA) or array (NumPy) [B, channels, H, W] to write into; its other channels keep their
        values.  Without `out` a CUDA tensor is made (a NumPy array with host=True; channels other than the three written are
        then uninitialised)."""
        owner, sp, smem, sh = self._u8_source(images)
        if len(sh) != 4 or sh[3] != 3:
            raise ValueError(f"images must be uint8 [B, H, W, 3], got {sh}")
        Bs, Hs, Ws = int(sh[0]), int(sh[1]), int(sh[2])
        H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
        B = Bs if batch is None else int(batch)
        if out is not None:
            if tuple(out.shape) != (B, out.shape[1], H, W):
                raise ValueError(f"out must be [{B}, C, {H}, {W}], got {tuple(out.shape)}")
            if _is_torch(out):
                import torch
                if out.dtype != torch.float32 or not out.is_contiguous():
                    raise ValueError("out must be a contiguous float32 tensor")
                dp, dmem = out.data_ptr(), PD_MEM_DEVICE if out.is_cuda else PD_MEM_HOST
            else:
                if out.dtype != np.float32 or not out.flags.c_contiguous:
                    raise ValueError("out must be a C-contiguous float32 array")
                dp, dmem = out.ctypes.data, PD_MEM_HOST
            channels = int(out.shape[1])
        else:
            dmem = PD_MEM_HOST if host else PD_MEM_DEVICE
            out, dp = _new_out((B, channels, H, W), device=None if host else self._torch_device())
        a = pd_image_load_args()
        a.src, a.Bs, a.Hs, a.Ws, a.mem_src = sp, Bs, Hs, Ws, smem
        a.dst, a.B, a.C, a.H, a.W, a.c_off, a.mem_dst = dp, B, channels, H, W, int(c_off), dmem
        a.filter, a.batch_mode = _filter_code(filter), IMAGE_BATCH_MODES[batch_mode]
        a.mul, a.add = float(mul), float(add)
        self._order_after_torch(PD_MEM_DEVICE if PD_MEM_DEVICE in (smem, dmem) else PD_MEM_HOST)
        self._check(self.lib.pd_image_load(self._h, C.byref(a)))
        del owner
        return out

    def image_store(self, x, *, mul: float = 1.0, add: float = 0.0, rounding: str = "nearest_even", host: bool = False):
        """float32 [B, C, H, W], C 1 or 3 (NumPy or torch) -> uint8 [B, H, W, C] (pd_image_store):
        min(max(x * mul + add, 0), 1) * 255 in float32, then rounding "nearest_even" (np.round) or "trunc" (astype(uint8)).
        A CUDA tensor comes out, a NumPy array with host=True."""
        b = _Buf(x)
        if b.owner.ndim != 4 or b.owner.shape[1] not in (1, 3):
            raise ValueError(f"x must be [B, 1 or 3, H, W], got {tuple(b.owner.shape)}")
        B, Cc, H, W = (int(v) for v in b.owner.shape)
        dmem = PD_MEM_HOST if host else PD_MEM_DEVICE
        out, dp = _new_out((B, H, W, Cc), np.uint8, None if host else (b.device or self._torch_device()))
        self._order_after_torch(PD_MEM_DEVICE if PD_MEM_DEVICE in (b.mem, dmem) else PD_MEM_HOST)
        self._check(self.lib.pd_image_store(self._h, b.ptr, B, Cc, H, W, b.mem, float(mul), float(add), IMAGE_ROUNDINGS[rounding], dp, dmem))
        return out

    # ------------------------------------------------------------------ Canny edge detector (pd_canny)
    def canny(self, images, low: float, high: float, *, out=None, c_off: int = 0, mul: float = 1.0, add: float = 0.0, host: bool = False):
        """cv2.Canny(img, low, high) (aperture 3, L1 magnitude; annotator/canny/__init__.py) on the device, byte for byte:
        uint8 pictures [B, H, W, C] with C 1 or 3, or [B, H, W] (NumPy, or a CPU / CUDA torch tensor) -> uint8 [B, H, W] of 0 / 255
        (pd_canny).  A CUDA tensor comes out; a NumPy array with host=True or for a NumPy input.  out: an existing contiguous
        float32 [B, Cf, H, W] (CUDA tensor, CPU tensor or NumPy array) whose channels c_off .. c_off + 2 also receive the edge map as
        (edge / 255) * mul + add in float32, replicated to three channels (HWC3 of the grey map); its other channels keep their
        values."""
        owner, sp, smem, sh = self._u8_source(images)
        if len(sh) == 3:
            sh = tuple(sh) + (1,)
        if len(sh) != 4:
            raise ValueError(f"images must be uint8 [B, H, W, C] or [B, H, W], got {tuple(sh)}")
        B, H, W, Cs = (int(v) for v in sh)   # pd_canny refuses a C other than 1 or 3
        a = pd_canny_args()
        a.src, a.B, a.H, a.W, a.C, a.mem_src = sp, B, H, W, Cs, smem
        a.low, a.high = float(low), float(high)
        any_dev = smem == PD_MEM_DEVICE
        if out is not None:
            if len(out.shape) != 4 or tuple(out.shape) != (B, out.shape[1], H, W):
                raise ValueError(f"out must be [{B}, Cf, {H}, {W}], got {tuple(out.shape)}")
            if _is_torch(out):
                import torch
                if out.dtype != torch.float32 or not out.is_contiguous():
                    raise ValueError("out must be a contiguous float32 tensor")
                a.dst_f, a.mem_f = out.data_ptr(), PD_MEM_DEVICE if out.is_cuda else PD_MEM_HOST
            else:
                if out.dtype != np.float32 or not out.flags.c_contiguous:
                    raise ValueError("out must be a C-contiguous float32 array")
                a.dst_f, a.mem_f = out.ctypes.data, PD_MEM_HOST
            a.Cf, a.c_off, a.mul, a.add = int(out.shape[1]), int(c_off), float(mul), float(add)
            any_dev = any_dev or a.mem_f == PD_MEM_DEVICE
        to_host = host or not _is_torch(images)
        edges, a.dst_u8 = _new_out((B, H, W), np.uint8, None if to_host else (owner.device if smem == PD_MEM_DEVICE else self._torch_device()))
        a.mem_u8 = PD_MEM_HOST if to_host else PD_MEM_DEVICE
        any_dev = any_dev or not to_host
        self._order_after_torch(PD_MEM_DEVICE if any_dev else PD_MEM_HOST)
        self._check(self.lib.pd_canny(self._h, C.byref(a)))
        del owner
        return edges

    def canny_hysteresis(self, states):
        """The hysteresis step alone on a state map (pd_op_canny_hysteresis): uint8 [B, H, W] of 0 (not a candidate), 1 (weak),
        2 (strong) -> the same map with every weak pixel 8-connected, through weak pixels, to a strong one set to 2.  NumPy in,
        NumPy out; CUDA tensor in, CUDA tensor out.  stat("canny_sweeps") holds the launches it took."""
        owner, sp, smem, sh = self._u8_source(states)
        if len(sh) != 3:
            raise ValueError(f"states must be uint8 [B, H, W], got {tuple(sh)}")
        out, op = _new_out(tuple(sh), np.uint8, owner.device if smem == PD_MEM_DEVICE else None)
        self._order_after_torch(smem)
        self._check(self.lib.pd_op_canny_hysteresis(self._h, sp, int(sh[0]), int(sh[1]), int(sh[2]), smem, op))
        del owner
        return out

    def text_weights_missing(self) -> int:
        return int(self.lib.pd_text_weights_missing(self._h))

    def text_encode(self, input_ids, clip_skip: int = 0):
        """FrozenCLIPEmbedder.forward after tokenisation (ldm/modules/encoders/modules.py:118-128): token ids
        [B, context_len] -> last_hidden_state [B, context_len, context_dim] fp32 (NumPy in, NumPy out; CUDA int32 tensor in,
        CUDA tensor out).  clip_skip k: hidden_states[-(k+1)] through final_layer_norm (pipeline_prompt_diffusion.py:398-413)."""
        clip_skip = int(clip_skip or 0)
        if _is_torch(input_ids):
            import torch
            ids = input_ids.to(torch.int32).contiguous()
            if ids.is_cuda:
                out, op = _new_out(tuple(ids.shape) + (self.cfg.context_dim,), device=ids.device)
                self._order_after_torch(PD_MEM_DEVICE)
                self._check(self.lib.pd_text_encode_ex(self._h, ids.data_ptr(), ids.shape[0], PD_MEM_DEVICE, clip_skip, op))
                return out
            input_ids = ids.numpy()
        ids = np.ascontiguousarray(input_ids, np.int32)
        if ids.ndim != 2 or ids.shape[1] != self.cfg.context_len:
            raise ValueError(f"input_ids must be [B, {self.cfg.context_len}]")
        out, op = _new_out(ids.shape + (self.cfg.context_dim,))
        self._check(self.lib.pd_text_encode_ex(self._h, ids.ctypes.data, ids.shape[0], PD_MEM_HOST, clip_skip, op))
        return out

    # ------------------------------------------------------------------ operator boundary
    def control_shapes(self, h: int, w: int) -> List[Tuple[int, int, int]]:
        out = []
        c, hh, ww = C.c_int32(), C.c_int32(), C.c_int32()
        n = len([0 for _ in range(PD_NUM_CONTROL)])
        from .weights import encoder_layout
        n = len(encoder_layout(self.cfg)) + 1
        for i in range(n):
            self._check(self.lib.pd_control_shape(self._h, i, h, w, C.byref(c), C.byref(hh), C.byref(ww)))
            out.append((c.value, hh.value, ww.value))
        return out

    def eps(self, x, t, ctx, pair, query, scales: Optional[Sequence[float]] = None, return_control: bool = False):
        """apply_model (cldm/cldm.py:369-382): eps [Bf,4,h,w] (and the 13 scaled control tensors).  ctx [Bf, L, context_dim] of any
        length L <= PD_MAX_CONTEXT_LEN."""
        xb, cb, pb, qb = _Buf(x), _Buf(ctx), _Buf(pair), _Buf(query)
        Bf, _, h, w = xb.owner.shape
        L = self._context_len(cb.owner, Bf, "ctx")
        mem = xb.mem
        if any(b.mem != mem for b in (cb, pb, qb)):
            raise PdError("all inputs must live in the same memory space")
        tb = _Buf(t, np.int64)
        if tb.mem != mem:
            raise PdError("t must live in the same memory space as x")
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float32)
        shapes = self.control_shapes(h, w)
        eps, ep = _new_out((Bf, self.cfg.out_channels, h, w), device=xb.device)
        res, rp = _new_out(sum(Bf * c * a * b for c, a, b in shapes), device=xb.device) if return_control else (None, None)
        self._order_after_torch(mem)
        self._check(self.lib.pd_eps_ctx(self._h, xb.ptr, tb.ptr, cb.ptr, L, pb.ptr, qb.ptr,
                                        None if sc is None else sc.ctypes.data, Bf, h, w, mem, ep, rp))
        if not return_control:
            return eps
        outs, off = [], 0
        for c, a, b in shapes:
            n = Bf * c * a * b
            outs.append(res[off:off + n].reshape(Bf, c, a, b))
            off += n
        return eps, outs

    def _context_len(self, ctx, batch: int, what: str) -> int:
        """L of a context tensor [batch, L, context_dim] (pd_sample_args.context_len)."""
        sh = tuple(ctx.shape)
        if len(sh) != 3 or sh[0] != batch or sh[2] != self.cfg.context_dim:
            raise ValueError(f"{what} must be [{batch}, L, {self.cfg.context_dim}], got {sh}")
        if not 1 <= sh[1] <= PD_MAX_CONTEXT_LEN:
            raise ValueError(f"{what}: context length {sh[1]} out of range 1 .. {PD_MAX_CONTEXT_LEN}")
        return int(sh[1])

    # ------------------------------------------------------------------ sampling
    def num_ddim_steps(self, steps: int) -> int:
        """len(make_ddim_timesteps('uniform')) -- may exceed `steps` (util.py:47-49)."""
        T = self.cfg.timesteps
        return len(range(0, T, T // steps))

    def make_schedule(self, steps: int, eta: float = 0.0) -> Dict[str, np.ndarray]:
        n = self.num_ddim_steps(steps)
        ts = np.zeros(n, np.int64)
        arrs = [np.zeros(n, np.float32) for _ in range(4)]
        self._check(self.lib.pd_make_schedule(self._h, steps, eta, ts.ctypes.data, *[a.ctypes.data for a in arrs]))
        return dict(ddim_timesteps=ts, ddim_alphas=arrs[0], ddim_alphas_prev=arrs[1], ddim_sigmas=arrs[2],
                    ddim_sqrt_one_minus_alphas=arrs[3])

    def _args(self, *, x_T, ctx_cond, ctx_uncond, pair, query, steps, cfg_scale, eta=0.0, use_cfg=True,
              guess_mode=False, only_mid_control=False, temperature=1.0, control_scales=None,
              control_scales_step=None, noise=None, pair_uncond=None, query_uncond=None, timesteps=None,
              init_latents=None, mask=None, init_pure_noise=False, seed_x_T=False):
        """noise="engine": the per-step draws (eta > 0 DDIM, multistep rows with a noise coefficient) come from the engine's
        generator (set_rng; PD_NOISE_FROM_SEED).  x_T=None with seed_x_T=True: the engine draws the start latents too
        (PD_XT_FROM_SEED); batch and latent size then come from init_latents, or from ctx_cond and pair.
        init_latents [B,4,h,w] (z0, already times scale_factor) turns x_T into the noise draw of img2img; mask [B,1,h,w] or
        [1,1,h,w] (1 = repaint) adds the inpainting blend after every step; init_pure_noise starts from x_T itself
        (pd_sample_args.init_latents / mask / init_flags).
        ctx_cond / ctx_uncond are [B, L, context_dim] with any equal L <= PD_MAX_CONTEXT_LEN (pd_sample_args.context_len)."""
        flags = PD_INIT_PURE_NOISE if init_pure_noise else 0
        if isinstance(noise, str):
            if noise != "engine":
                raise ValueError("noise must be an array or \"engine\"")
            noise, flags = None, flags | PD_NOISE_FROM_SEED
        if seed_x_T:
            if x_T is not None:
                raise PdError("seed_x_T: x_T must be None (PD_XT_FROM_SEED: the engine draws it)")
            flags |= PD_XT_FROM_SEED
            xs = tuple(init_latents.shape) if init_latents is not None else \
                (ctx_cond.shape[0], self.cfg.in_channels, pair.shape[2] // 8, pair.shape[3] // 8)
        elif x_T is None:
            raise PdError("x_T is required (or seed_x_T=True for the engine's own draw)")
        else:
            xs = tuple(x_T.shape)
        if mask is not None:
            B0 = xs[0]
            if tuple(mask.shape[1:]) != (1,) + xs[2:] or mask.shape[0] not in (1, B0):
                raise PdError(f"mask must be [B, 1, h, w] or [1, 1, h, w] with B, h, w of x_T {xs}, got {tuple(mask.shape)}")
            if mask.shape[0] != B0:      # broadcast over the batch on the host side of the boundary
                mask = mask.expand(B0, -1, -1, -1) if _is_torch(mask) else np.broadcast_to(mask, (B0,) + tuple(mask.shape[1:]))
        bufs = dict(x_T=_Buf(x_T), ctx_cond=_Buf(ctx_cond), ctx_uncond=_Buf(ctx_uncond), pair=_Buf(pair),
                    query=_Buf(query), pair_uncond=_Buf(pair_uncond), query_uncond=_Buf(query_uncond), noise=_Buf(noise),
                    init_latents=_Buf(init_latents), mask=_Buf(mask))
        mems = {b.mem for b in bufs.values() if b.mem is not None}
        if len(mems) != 1:
            raise PdError("all inputs must live in the same memory space (all NumPy or all CUDA tensors)")
        if init_latents is not None and tuple(init_latents.shape) != xs:
            raise PdError(f"init_latents must have the shape of x_T {xs}, got {tuple(init_latents.shape)}")
        a = pd_sample_args()
        a.init_flags = flags
        B, _, h, w = xs
        a.context_len = self._context_len(bufs["ctx_cond"].owner, B, "ctx_cond")
        cu = bufs["ctx_uncond"].owner
        if cu is not None and tuple(cu.shape) != tuple(bufs["ctx_cond"].owner.shape):
            # (the reference's torch.cat of the two halves, ddim_hacked.py:191, raises as well)
            raise ValueError(f"ctx_uncond {tuple(cu.shape)} must have the shape of ctx_cond {tuple(bufs['ctx_cond'].owner.shape)}")
        a.batch, a.h, a.w, a.steps = B, h, w, steps
        a.eta, a.cfg_scale, a.use_cfg = eta, cfg_scale, 1 if use_cfg else 0
        a.guess_mode, a.only_mid_control, a.temperature = int(guess_mode), int(only_mid_control), temperature
        a.mem = mems.pop()
        for k, b in bufs.items():
            setattr(a, k, b.ptr)
        keep = [bufs["ctx_cond"]] + list(bufs.values())    # keep[0]: an input that always exists (memory space / device of the outputs)
        n_steps = self.num_ddim_steps(steps)
        if timesteps is not None:       # custom grid, sampling order (descending); a.steps = its length
            ts = np.ascontiguousarray(_to_host(timesteps), dtype=np.int64).reshape(-1)
            a.steps = n_steps = len(ts)
            a.timesteps = ts.ctypes.data
            keep.append(ts)
        if control_scales is not None:
            cs = np.zeros(PD_NUM_CONTROL, np.float32)
            cs[:len(control_scales)] = control_scales
            a.control_scales = cs.ctypes.data
            keep.append(cs)
        if control_scales_step is not None:
            css = np.ascontiguousarray(control_scales_step, dtype=np.float32)
            assert css.shape == (n_steps, PD_NUM_CONTROL)
            a.control_scales_step = css.ctypes.data
            keep.append(css)
        self._order_after_torch(a.mem)
        return a, keep, (B, h, w)

    def _sample_out(self, a, keep, B, h, w, S, return_intermediates):
        """out [B,4,h,w] and optionally inter [S+1,B,4,h,w] in the memory space of the inputs, and their addresses."""
        Cc = self.cfg.in_channels
        dev = keep[0].owner.device if a.mem == PD_MEM_DEVICE else None
        out, op = _new_out((B, Cc, h, w), device=dev)
        inter, ip = _new_out((S + 1, B, Cc, h, w), device=dev) if return_intermediates else (None, None)
        return out, inter, op, ip

    def ddim_sample(self, *, return_intermediates: bool = False, **kw):
        """The fused loop (DDIMSampler.sample, cldm/ddim_hacked.py:55-178): returns latents [B,4,h,w]
        (NumPy, or a CUDA tensor when the inputs were CUDA tensors) and optionally x_inter [S+1,B,4,h,w]."""
        a, keep, (B, h, w) = self._args(**kw)
        S = a.steps if a.timesteps else self.num_ddim_steps(a.steps)
        out, inter, op, ip = self._sample_out(a, keep, B, h, w, S, return_intermediates)
        self._check(self.lib.pd_ddim_sample(self._h, C.byref(a), a.mem, op, ip))
        del keep
        return (out, inter) if return_intermediates else out

    def unipc_sample(self, *, return_intermediates: bool = False, order: int = 2, solver_type: str = "bh2",
                     lower_order_final: bool = True, disable_corrector: Sequence[int] = (), **kw):
        """The fused UniPC loop (the update of schedulers.UniPCMultistepScheduler, run on the device): `timesteps` (the grid,
        sampling order) is required; otherwise the arguments and returns of ddim_sample."""
        a, keep, (B, h, w) = self._args(**kw)
        u, dc = _unipc_args(order, solver_type, lower_order_final, disable_corrector)
        out, inter, op, ip = self._sample_out(a, keep, B, h, w, a.steps, return_intermediates)
        self._check(self.lib.pd_unipc_sample(self._h, C.byref(a), C.byref(u), a.mem, op, ip))
        del keep, dc
        return (out, inter) if return_intermediates else out

    def _lms_call(self, kw, kind, order, solver_type, lower_order_final, model_times, rows, row_times):
        """pd_sample_args + pd_lms_args of a linear multistep call; the step count comes from the grid."""
        kw = dict(kw)
        kw["steps"] = n = _lms_steps(kw.get("timesteps"), model_times, kw.get("steps"))
        if kind == "euler_a" and kw.get("noise") is None:
            kw["noise"] = "engine"     # an ancestral sampler always draws; the only source is the engine's generator
        css = kw.pop("control_scales_step", None)      # one row per sampling step of this grid, not of a DDIM schedule
        a, keep, shape = self._args(**kw)
        a.steps = n
        if css is not None:
            css = np.ascontiguousarray(css, dtype=np.float32)
            if css.shape != (n, PD_NUM_CONTROL):
                raise PdError(f"control_scales_step must be [{n}, {PD_NUM_CONTROL}], got {css.shape}")
            a.control_scales_step = css.ctypes.data
            keep.append(css)
        u, lkeep = _lms_args(kind, order, solver_type, lower_order_final, model_times, rows, row_times)
        return a, keep + lkeep, shape, u

    def lms_sample(self, *, return_intermediates: bool = False, kind: str = "dpmsolver++", order: int = 2,
                   solver_type: str = "dpm_solver", lower_order_final: bool = True, model_times=None, rows=None, row_times=None,
                   **kw):
        """The fused linear multistep loop (PLMS, DPM-Solver++ multistep, Euler ancestral -- kind "euler_a", whose noise the
        engine draws (set_rng) --, or the caller's own rows, with noise="engine" when they carry a noise coefficient; see lms_coefficients):
        `timesteps` or `model_times` is the grid; otherwise the arguments and returns of ddim_sample.  x_inter has one entry
        per completed step, however many evaluations ran."""
        a, keep, (B, h, w), u = self._lms_call(kw, kind, order, solver_type, lower_order_final, model_times, rows, row_times)
        out, inter, op, ip = self._sample_out(a, keep, B, h, w, a.steps, return_intermediates)
        self._check(self.lib.pd_lms_sample(self._h, C.byref(a), C.byref(u), a.mem, op, ip))
        del keep
        return (out, inter) if return_intermediates else out

    def lms_coefficients(self, timesteps=None, **kw):
        return lms_coefficients(self.cfg, timesteps, **kw)

    def sample_begin_lms(self, *, kind: str = "dpmsolver++", order: int = 2, solver_type: str = "dpm_solver",
                         lower_order_final: bool = True, model_times=None, rows=None, row_times=None, **kw) -> int:
        """Stepwise form of lms_sample; returns the number of rows: sample_step(i) runs evaluation i."""
        a, keep, shape, u = self._lms_call(kw, kind, order, solver_type, lower_order_final, model_times, rows, row_times)
        self._check(self.lib.pd_sample_begin_lms(self._h, C.byref(a), C.byref(u)))
        self._session_begun(a, keep, shape)
        return int(self.lib.pd_sample_rows(self._h))

    def _session_begun(self, a, keep, shape) -> None:
        self._keep = keep   # the staged copies stay alive until sample_end()
        self._ses = (shape, a.mem, keep[0].owner if a.mem == PD_MEM_DEVICE else None)

    def sample_begin_unipc(self, *, order: int = 2, solver_type: str = "bh2", lower_order_final: bool = True,
                           disable_corrector: Sequence[int] = (), **kw) -> int:
        """Stepwise form of unipc_sample: then sample_step / sample_get / sample_set_latents / sample_end."""
        a, keep, shape = self._args(**kw)
        u, dc = _unipc_args(order, solver_type, lower_order_final, disable_corrector)
        self._check(self.lib.pd_sample_begin_unipc(self._h, C.byref(a), C.byref(u)))
        del dc
        self._session_begun(a, keep, shape)
        return a.steps

    def sample_begin(self, **kw) -> int:
        a, keep, shape = self._args(**kw)
        self._check(self.lib.pd_sample_begin(self._h, C.byref(a)))
        self._session_begun(a, keep, shape)
        return a.steps if a.timesteps else self.num_ddim_steps(a.steps)

    def sample_step(self, i: int) -> None:
        self._check(self.lib.pd_sample_step(self._h, i))

    def sample_get(self, what: int = PD_GET_LATENTS):
        (B, h, w), mem, like = self._ses
        out, op = _new_out((B, self.cfg.in_channels, h, w), device=like.device if mem == PD_MEM_DEVICE else None)
        self._check(self.lib.pd_sample_get(self._h, what, mem, op))
        return out

    def sample_set_latents(self, latents) -> None:
        b = _Buf(latents)
        self._order_after_torch(b.mem)
        self._check(self.lib.pd_sample_set_latents(self._h, b.mem, b.ptr))

    def sample_set_guidance(self, scale: float) -> None:
        """unconditional_guidance_scale of the following steps (ucg_schedule, cldm/ddim_hacked.py:159-161)."""
        self._check(self.lib.pd_sample_set_guidance(self._h, float(scale)))

    def sample_eps_at(self, t: int, scales: Optional[Sequence[float]] = None):
        sc = None
        if scales is not None:
            sc = np.zeros(PD_NUM_CONTROL, np.float32)
            sc[:len(scales)] = scales
        self._check(self.lib.pd_sample_eps_at(self._h, int(t), None if sc is None else sc.ctypes.data))
        return self.sample_get(PD_GET_EPS)

    def sample_end(self) -> None:
        self._check(self.lib.pd_sample_end(self._h))
        self._keep = []

    # ------------------------------------------------------------------ multi-GPU
    def comm_new_id(self) -> bytes:
        """The 128-byte rendezvous token rank 0 creates and hands to every rank (any host channel)."""
        buf = (C.c_uint8 * PD_COMM_ID_BYTES)()
        self._check(self.lib.pd_comm_new_id(buf))
        return bytes(buf)

    def comm_init(self, comm_id: bytes, world: int, rank: int) -> None:
        """Join the engine-owned RCCL communicator (collective over all `world` ranks; one process and one engine per GPU)."""
        if len(comm_id) != PD_COMM_ID_BYTES:
            raise ValueError("comm_id must be the %d bytes of comm_new_id()" % PD_COMM_ID_BYTES)
        buf = (C.c_uint8 * PD_COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._check(self.lib.pd_comm_init(self._h, buf, int(world), int(rank)))

    def comm_world(self) -> Tuple[int, int]:
        w, r = C.c_int32(), C.c_int32()
        self._check(self.lib.pd_comm_world(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def comm_all_gather(self, latents):
        """[b, ...] from every rank -> [world * b, ...] in rank order (equal b on every rank); the path's only exchange."""
        world, _ = self.comm_world()
        b = _Buf(latents)
        self._order_after_torch(b.mem)
        shape = (world * b.owner.shape[0],) + tuple(b.owner.shape[1:])
        count = int(np.prod(b.owner.shape))
        out, op = _new_out(shape, device=b.device)
        self._check(self.lib.pd_comm_all_gather(self._h, b.ptr, op, count, b.mem))
        return out

    def comm_destroy(self) -> None:
        self._check(self.lib.pd_comm_destroy(self._h))

    # ------------------------------------------------------------------ instrumentation
    def synchronize(self):
        self._check(self.lib.pd_synchronize(self._h))

    def stat(self, key: str) -> int:
        return int(self.lib.pd_get_stat(self._h, key.encode()))

    def set_option(self, key: str, value: int):
        self._check(self.lib.pd_set_option(self._h, key.encode(), int(value)))

    def option(self, key: str) -> int:
        """The value the option holds now, as set_option stored it (pd_get_option): save it, flip the knob, put it back."""
        v = C.c_int64()
        self._check(self.lib.pd_get_option(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def profile_read(self, klass: int = -1) -> Tuple[float, int, float]:
        """(device ms, launches, algorithmic FLOPs) of the launches bracketed while option 'profile' was on."""
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._check(self.lib.pd_profile_read(self._h, klass, C.byref(ms), C.byref(n), C.byref(fl)))
        return float(ms.value), int(n.value), float(fl.value)

    def profile_dump(self, path: str) -> None:
        self._check(self.lib.pd_profile_dump(self._h, path.encode()))

    def bench_conv3x3(self, Bf: int, H: int, W: int, Cin: int, Cout: int, iters: int = 20) -> float:
        ms = C.c_float()
        self._check(self.lib.pd_bench_conv3x3(self._h, Bf, H, W, Cin, Cout, iters, C.byref(ms)))
        return float(ms.value)

    def bench_linear(self, M: int, K: int, N: int, residual: bool = False, iters: int = 20) -> float:
        ms = C.c_float()
        self._check(self.lib.pd_bench_linear(self._h, M, K, N, 1 if residual else 0, iters, C.byref(ms)))
        return float(ms.value)

    # ------------------------------------------------------------------ per-op parity hooks
    def op_conv2d(self, x, w, b=None, residual=None, stride=1, upsample=False, silu=False, scale=1.0, stream_out=False):
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        B, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        Hv, Wv = (H * 2, W * 2) if upsample else (H, W)
        Ho, Wo = ((Hv + 1) // 2, (Wv + 1) // 2) if stride == 2 else (Hv, Wv)
        y = np.empty((B, Cout, Ho, Wo), np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        rr = None if residual is None else np.ascontiguousarray(residual, np.float32)
        self._check(self.lib.pd_op_conv2d(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data,
                                          None if rr is None else rr.ctypes.data, B, Cin, H, W, Cout, k, stride,
                                          int(upsample), int(silu), scale, int(stream_out), y.ctypes.data))
        return y

    def op_conv2d_upfold(self, x, w, b=None, residual=None):
        """conv3x3(nearest_x2(x)) through the weight fold and the four-phase kernel (option 'ups_fold'); raises where the dispatch
        would not take that kernel instead of falling back."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        assert w.shape == (Cout, Cin, 3, 3), w.shape
        y = np.empty((B, Cout, 2 * H, 2 * W), np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        rr = None if residual is None else np.ascontiguousarray(residual, np.float32)
        self._check(self.lib.pd_op_conv2d_upfold(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data,
                                                 None if rr is None else rr.ctypes.data, B, Cin, H, W, Cout, y.ctypes.data))
        return y

    def op_linear(self, x, w, b=None, geglu=False, a_silu=False):
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        M, K = x.shape
        N = w.shape[0] // 2 if geglu else w.shape[0]
        y = np.empty((M, N), np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        self._check(self.lib.pd_op_linear(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data,
                                          M, K, N, int(geglu), int(a_silu), y.ctypes.data))
        return y

    DTYPE_CODES = {"f32": 0, "T": 1, "S": 2}     # pd_gemm_ex_args.res_dt / out_dt: fp32, the compute type, the residual-stream type

    def op_linear_ex(self, x, w, b=None, act: int = 0, a_silu: bool = False, scale: float = 1.0, residual=None, res_dt: str = "f32",
                     out_dt: str = "f32", rows_per_sample: int = 0, rowvec=None, gate=None, vt_begin: int = 0, vt_extra: int = 0,
                     vt_tok_off: int = 0, c_sample_rows: int = 0, c_row_off: int = 0, a_sample_rows: int = 0, a_row_off: int = 0,
                     ldc_extra: int = 0, ln=None):
        """pd_engine::gemm on a linear layer in the forms its callers launch (pd_op_linear_ex): x [M, K], w [N, K] (act 2 / 7: [2N, K]
        packed [x | gate]) -> (y [M, N or vt_begin], vt [B, N - vt_begin, tokens] or None, touched).  act: Activation of pd_common.h;
        residual [M, N] held in res_dt; out_dt the type of C and V^T ("f32", "T" compute type, "S" stream type); rows_per_sample: tokens
        per sample (M = B x tokens); rowvec, gate [B, N]; the columns >= vt_begin go transposed to vt, behind vt_tok_off tokens and with
        vt_extra more pad tokens per row; c_ / a_sample_rows, _row_off: the rows of C / A sit at b * sample_rows + row_off + t of a joint
        buffer; ldc_extra: more output row stride; ln = (gamma, beta): LayerNorm(x) folded into the layer.  Every output buffer is
        filled with NaN first; touched counts the elements outside the call's own that the launch changed.  Stats "gemm_family",
        "gemm_tile", "gemm_splitk" say which kernel ran."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        x, w, b, residual, rowvec, gate = (f(a) for a in (x, w, b, residual, rowvec, gate))
        lg, lb = (f(ln[0]), f(ln[1])) if ln is not None else (None, None)
        M, K = x.shape
        packed = act in (2, 7)
        N = w.shape[0] // 2 if packed else w.shape[0]
        tokens = rows_per_sample or M
        B = M // tokens
        if w.shape != ((2 * N if packed else N), K) or (b is not None and b.shape != (w.shape[0],)) or (residual is not None and residual.shape != (M, N)) \
                or any(a is not None and a.shape != (B, N) for a in (rowvec, gate)) or (ln is not None and (lg.shape != (K,) or lb.shape != (K,))):
            raise ValueError("x [M, K], w [N, K], b [N], residual [M, N], rowvec / gate [B, N], ln ([K], [K])")
        y = np.empty((M, N), np.float32)
        vt = np.empty((B, N - vt_begin, tokens), np.float32) if vt_begin else None
        p = lambda a: None if a is None else a.ctypes.data
        a = pd_gemm_ex_args(x=p(x), w=p(w), bias=p(b), residual=p(residual), rowvec=p(rowvec), gate=p(gate), ln_gamma=p(lg), ln_beta=p(lb),
                            M=M, K=K, N=N, act=int(act), a_silu=int(bool(a_silu)), res_dt=self.DTYPE_CODES[res_dt], out_dt=self.DTYPE_CODES[out_dt],
                            rows_per_sample=int(rows_per_sample), vt_begin=int(vt_begin), vt_extra=int(vt_extra), vt_tok_off=int(vt_tok_off),
                            c_sample_rows=int(c_sample_rows), c_row_off=int(c_row_off), a_sample_rows=int(a_sample_rows), a_row_off=int(a_row_off),
                            ldc_extra=int(ldc_extra), scale=float(scale), y=p(y), vt=p(vt), touched=0)
        self._check(self.lib.pd_op_linear_ex(self._h, C.byref(a)))
        return (y[:, :vt_begin] if vt_begin else y), vt, int(a.touched)

    def op_conv2d_ex(self, x, w, b=None, residual=None, rowvec=None, stride=1, upsample=False, act: int = 0, scale=1.0, stream_out=False):
        """op_conv2d plus rowvec [B, Cout] (the per-sample time-embedding row, added before the activation) and act 0 / 1 / 5 (none /
        SiLU / ReLU) (pd_op_conv2d_ex)."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        B, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        Hv, Wv = (H * 2, W * 2) if upsample else (H, W)
        Ho, Wo = ((Hv + 1) // 2, (Wv + 1) // 2) if stride == 2 else (Hv, Wv)
        y = np.empty((B, Cout, Ho, Wo), np.float32)
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        bb, rr, rv = f(b), f(residual), f(rowvec)
        if rv is not None and rv.shape != (B, Cout):
            raise ValueError("rowvec [B, Cout]")
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.pd_op_conv2d_ex(self._h, x.ctypes.data, w.ctypes.data, p(bb), p(rr), p(rv), B, Cin, H, W, Cout, k, stride,
                                             int(upsample), int(act), scale, int(stream_out), y.ctypes.data))
        return y

    def op_linear_fp8(self, x, w, b=None, gelu_tanh=False):
        """The SD3 path's e4m3 linear layer (per-row scales of x and w) on host arrays."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        M, K = x.shape
        N = w.shape[0]
        y = np.empty((M, N), np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        self._check(self.lib.pd_op_linear_fp8(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data, M, K, N,
                                              4 if gelu_tanh else 0, y.ctypes.data))
        return y

    def op_groupnorm(self, x, gamma, beta, eps=1e-5, silu=False):
        x = np.ascontiguousarray(x, np.float32)
        g = np.ascontiguousarray(gamma, np.float32); b = np.ascontiguousarray(beta, np.float32)
        B, Cc, H, W = x.shape
        y = np.empty_like(x)
        self._check(self.lib.pd_op_groupnorm(self._h, x.ctypes.data, g.ctypes.data, b.ctypes.data, B, Cc, H, W, eps,
                                             int(silu), y.ctypes.data))
        return y

    def op_layernorm(self, x, gamma, beta):
        x = np.ascontiguousarray(x, np.float32)
        g = np.ascontiguousarray(gamma, np.float32); b = np.ascontiguousarray(beta, np.float32)
        rows, Cc = x.shape
        y = np.empty_like(x)
        self._check(self.lib.pd_op_layernorm(self._h, x.ctypes.data, g.ctypes.data, b.ctypes.data, rows, Cc, y.ctypes.data))
        return y

    def op_groupnorm_slabs(self, slabs, gamma, beta, bias=None, row=None, eps=1e-5, silu=False):
        """GroupNorm32 of round(slab_0 + slab_1 + ... + bias + row): slabs [nslab, B, H, W, C] (channels last), bias [C], row [B, C]
        -> [B, C, H, W] (pd_op_groupnorm_slabs)."""
        slabs = np.ascontiguousarray(slabs, np.float32)
        nslab, B, H, W, Cc = slabs.shape
        g = np.ascontiguousarray(gamma, np.float32); b = np.ascontiguousarray(beta, np.float32)
        bb = None if bias is None else np.ascontiguousarray(bias, np.float32)
        rr = None if row is None else np.ascontiguousarray(row, np.float32)
        assert g.shape == (Cc,) and b.shape == (Cc,) and (bb is None or bb.shape == (Cc,)) and (rr is None or rr.shape == (B, Cc))
        y = np.empty((B, Cc, H, W), np.float32)
        self._check(self.lib.pd_op_groupnorm_slabs(self._h, slabs.ctypes.data, nslab, None if bb is None else bb.ctypes.data,
                                                   None if rr is None else rr.ctypes.data, g.ctypes.data, b.ctypes.data, B, Cc, H, W, eps,
                                                   int(silu), y.ctypes.data))
        return y

    def op_groupnorm_coef(self, x, gamma, beta, eps=1e-5):
        """The {a, b} of GroupNorm32(x) = x * a + b per (sample, channel): [B, C, 2] (pd_op_groupnorm_coef)."""
        x = np.ascontiguousarray(x, np.float32)
        g = np.ascontiguousarray(gamma, np.float32); b = np.ascontiguousarray(beta, np.float32)
        B, Cc, H, W = x.shape
        assert g.shape == (Cc,) and b.shape == (Cc,)
        coef = np.empty((B, Cc, 2), np.float32)
        self._check(self.lib.pd_op_groupnorm_coef(self._h, x.ctypes.data, g.ctypes.data, b.ctypes.data, B, Cc, H, W, eps, coef.ctypes.data))
        return coef

    def op_ln_linear(self, mode, gamma, beta, w, bias=None, h=None, x=None, w1=None, b1=None, residual=None):
        """Linear(LayerNorm(h)) (pd_op_ln_linear): mode 0 the kernel pair, 1 the fold with row_stats_kernel's statistics (both on h
        [M, K]), 2 the fold behind the producer h = x @ w1.T + b1 (+ residual).  Returns (y [M, N], h as the consumer read it,
        statistics partials per row that fed the fold, their per-row sums [M, 2] = {sum, sum of squares})."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        g, b, w, bias, h, x, w1, b1, residual = (f(a) for a in (gamma, beta, w, bias, h, x, w1, b1, residual))
        N, K = w.shape
        src = x if mode == 2 else h
        M = src.shape[0]
        assert src.shape == (M, K) and g.shape == (K,) and b.shape == (K,) and (bias is None or bias.shape == (N,))
        if mode == 2:
            assert w1.shape == (K, K) and (b1 is None or b1.shape == (K,)) and (residual is None or residual.shape == (M, K))
        p = lambda a: None if a is None else a.ctypes.data
        y = np.empty((M, N), np.float32)
        h_out = np.empty((M, K), np.float32)
        parts = C.c_int(0)
        row_stats = np.zeros((M, 2), np.float32)
        self._check(self.lib.pd_op_ln_linear(self._h, int(mode), p(h), p(x), p(w1), p(b1), p(residual), p(g), p(b), p(w), p(bias), M, K, N,
                                             h_out.ctypes.data, y.ctypes.data, C.byref(parts), row_stats.ctypes.data))
        return y, h_out, int(parts.value), row_stats

    def op_time_embed(self, t, net: int = 0, want_emb: bool = True):
        """(timestep_embedding(t, model_channels), time_embed(...)) of the loaded UNet (net 0) / ControlNet (net 1)."""
        t = np.ascontiguousarray(t, np.int64)
        mc = self.cfg.model_channels
        temb = np.empty((t.size, mc), np.float32)
        emb = np.empty((t.size, 4 * mc), np.float32) if want_emb else None
        self._check(self.lib.pd_op_time_embed(self._h, int(net), t.ctypes.data, int(t.size), temb.ctypes.data, emb.ctypes.data if want_emb else None))
        return temb, emb

    def op_attention(self, q, k, v):
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        B, Nq, Cc = q.shape
        Nk = k.shape[1]
        o = np.empty_like(q)
        self._check(self.lib.pd_op_attention(self._h, q.ctypes.data, k.ctypes.data, v.ctypes.data, B, Nq, Nk, Cc, o.ctypes.data))
        return o

    def op_attention_ex(self, q, k, v, heads: int = 0, causal: bool = False, scale: float = 0.0, relbias=None, layout: int = 0,
                        vt_extra: int = 0, pad_fill: float = 0.0):
        """pd_engine::attention in the forms its callers launch (pd_op_attention_ex): q [B, Nq, C], k, v [B, Nk, C] -> (o [B, Nq, C],
        touched).  heads 0: the config's; scale 0: dh^-0.5; relbias [heads, 2 Nk - 1] in natural-log units (dh 64, Nq == Nk, not causal);
        layout 1: q | k as rows of one [B, Nk, 2C] buffer, the queries its first Nq rows, the output buffer [B, Nk, C]; vt_extra: more V^T
        row padding (a multiple of 8 keys); pad_fill: what every pad column of V^T and, in layout 1, the q rows >= Nq and the output
        buffer hold before the launch.  touched: elements of the output rows >= Nq the launch changed (layout 1).  Stat "attn_kernel"
        says which kernel family ran."""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        B, Nq, Cc = q.shape
        Nk = k.shape[1]
        if k.shape != (B, Nk, Cc) or v.shape != k.shape:
            raise ValueError("q [B, Nq, C], k and v [B, Nk, C]")
        h = int(heads) if heads else self.cfg.num_heads
        rb = None
        if relbias is not None:
            rb = np.ascontiguousarray(relbias, np.float32)
            if rb.shape != (h, 2 * Nk - 1):
                raise ValueError("relbias must be [heads, 2 Nk - 1]")
        o = np.empty_like(q)
        touched = C.c_int64(0)
        self._check(self.lib.pd_op_attention_ex(self._h, q.ctypes.data, k.ctypes.data, v.ctypes.data, B, Nq, Nk, Cc, int(heads), int(bool(causal)),
                                                float(scale), None if rb is None else rb.ctypes.data, int(layout), int(vt_extra), float(pad_fill),
                                                o.ctypes.data, C.byref(touched)))
        return o, int(touched.value)

    def op_vae_attention(self, q, k, v):
        """softmax(q k^T C^-0.5) v with one head over all C channels (the first stage's AttnBlock); q, k, v [B, N, C].  Option
        "vae_flash" 1: the single-head flash kernel (2-byte modes, C 128 / 512); 0: the materialised three-launch path."""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        B, N, Cc = q.shape
        if k.shape != q.shape or v.shape != q.shape:
            raise ValueError("q, k and v must share one shape [B, N, C]")
        o = np.empty_like(q)
        self._check(self.lib.pd_op_vae_attention(self._h, q.ctypes.data, k.ctypes.data, v.ctypes.data, B, N, Cc, o.ctypes.data))
        return o

    def op_vae_downsample(self, x, w, b=None):
        """Downsample.forward (model.py:80-88): F.pad(x, (0,1,0,1)) then conv3x3 stride 2, padding 0; x [B,C,H,W] -> [B,C,H//2,W//2]."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        B, Cc, H, W = x.shape
        y = np.empty((B, Cc, H // 2, W // 2), np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        self._check(self.lib.pd_op_vae_downsample(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data,
                                                  B, Cc, H, W, y.ctypes.data))
        return y

    def op_hed_stage_tail(self, x, w, b, pool: bool = True):
        """One stage tail of the HED detector (hed_stage_tail_kernel) in the compute type: x [B,C,H,W], w [C] (or [1,C,1,1]), b [1] ->
        (score [B,H,W], max_pool2d(x, 2, 2) [B,C,H//2,W//2] or None)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1))
        bb = np.ascontiguousarray(np.asarray(b, np.float32).reshape(-1))
        B, Cc, H, W = x.shape
        if w.size != Cc or bb.size != 1:
            raise ValueError("w must hold C values and b one")
        score = np.empty((B, H, W), np.float32)
        pooled = np.empty((B, Cc, H // 2, W // 2), np.float32) if pool else None
        self._check(self.lib.pd_op_hed_stage_tail(self._h, x.ctypes.data, w.ctypes.data, bb.ctypes.data, B, Cc, H, W, score.ctypes.data,
                                                  None if pooled is None else pooled.ctypes.data))
        return score, pooled

    def op_hed_fuse(self, scores, cw, cb, what: str = "edge"):
        """The end of the HED detector (hed_fuse_kernel): scores = five maps [B,H>>i,W>>i] (or [B,1,H>>i,W>>i]), cw [5], cb [1] ->
        "edge" [B,1,H,W] = sigmoid(cb + sum_i cw[i] up_i) or "sides" [B,5,H,W] = the bilinear upsamples up_i."""
        maps = [np.ascontiguousarray(s, np.float32) for s in scores]
        if len(maps) != 5:
            raise ValueError("five score maps expected")
        B, H, W = maps[0].shape[0], maps[0].shape[-2], maps[0].shape[-1]
        for i, m in enumerate(maps):
            if m.size != B * (H >> i) * (W >> i) or m.shape[-1] != W >> i:
                raise ValueError(f"score map {i} must be [{B}, {H >> i}, {W >> i}]")
        flat = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in maps]))
        cw = np.ascontiguousarray(np.asarray(cw, np.float32).reshape(-1))
        cb = np.ascontiguousarray(np.asarray(cb, np.float32).reshape(-1))
        if cw.size != 5 or cb.size != 1:
            raise ValueError("cw must hold 5 values and cb one")
        out = np.empty((B, 5 if what == "sides" else 1, H, W), np.float32)
        self._check(self.lib.pd_op_hed_fuse(self._h, flat.ctypes.data, cw.ctypes.data, cb.ctypes.data, B, H, W, HED_OUTPUTS[what],
                                            out.ctypes.data))
        return out

    def op_dwconv3x3(self, x, w, b, stride: int = 1, in_relu6: bool = False):
        """The M-LSD depthwise conv3x3 + bias + ReLU6 (mlsd_dwconv_kernel) in the compute type: x [B,C,H,W], w [C,1,3,3], b [C] ->
        [B,C,Ho,Wo]; stride 2 pads a zero row / column at the bottom / right only.  in_relu6: min(max(x, 0), 6) while loading."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(b, np.float32).reshape(-1))
        B, Cc, H, W = x.shape
        if w.size != Cc * 9 or b.size != Cc:
            raise ValueError("w must be [C, 1, 3, 3] and b [C]")
        y = np.empty((B, Cc, H // stride, W // stride), np.float32)
        self._check(self.lib.pd_op_dwconv3x3(self._h, x.ctypes.data, w.ctypes.data, b.ctypes.data, B, Cc, H, W, int(stride), int(bool(in_relu6)),
                                             y.ctypes.data))
        return y

    def op_upcat_bilinear(self, x, y, c_off: int):
        """The M-LSD upsample into a concat buffer (mlsd_upcat_kernel): x [B,C,h,w] -> channels c_off .. c_off + C - 1 of a copy of
        y [B,Cy,2h,2w] (stored in the compute type), which is returned; its other channels come back as they went in."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.array(y, np.float32, order="C")
        B, Cc, h, w = x.shape
        if y.shape != (B, y.shape[1], 2 * h, 2 * w):
            raise ValueError(f"y must be [{B}, Cy, {2 * h}, {2 * w}]")
        self._check(self.lib.pd_op_upcat_bilinear(self._h, x.ctypes.data, B, Cc, h, w, int(y.shape[1]), int(c_off), y.ctypes.data))
        return y

    def op_conv2d_dilated(self, x, w, b, dilation: int, relu: bool = False):
        """nn.Conv2d(Cin, Cout, 3, padding=dilation, dilation=dilation) (+ ReLU) through the engine's dispatch."""
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        B, Cin, H, W = x.shape
        y = np.empty((B, w.shape[0], H, W), np.float32)
        self._check(self.lib.pd_op_conv2d_dilated(self._h, x.ctypes.data, w.ctypes.data, None if bb is None else bb.ctypes.data, B, Cin, H, W,
                                                  int(w.shape[0]), int(dilation), int(bool(relu)), y.ctypes.data))
        return y

    def op_mlsd_decode(self, tp, thr_v: float, thr_d: float):
        """pred_lines' decode (mlsd_peaks_kernel + mlsd_select_kernel) of tp [B,9,h,w] float32 -> a list of int32 [n_b, 4] per image."""
        tp = np.ascontiguousarray(tp, np.float32)
        B, nine, h, w = tp.shape
        if nine != 9:
            raise ValueError("tp must be [B, 9, h, w]")
        segs = np.zeros((B, MLSD_TOPK, 4), np.int32)
        count = np.zeros(B, np.int32)
        self._check(self.lib.pd_op_mlsd_decode(self._h, tp.ctypes.data, B, h, w, float(thr_v), float(thr_d), segs.ctypes.data, count.ctypes.data))
        return [segs[b, :int(count[b])].copy() for b in range(B)]

    def op_draw_lines(self, segs, H: int, W: int):
        """cv2.line(thickness 1) of every segment (mlsd_draw_kernel): segs = one int [n_b, 4] array per image -> uint8 [B, H, W]."""
        segs = [np.asarray(s, np.int32).reshape(-1, 4) for s in segs]
        B, n = len(segs), max(1, max(len(s) for s in segs))
        flat = np.zeros((B, n, 4), np.int32)
        for b, s in enumerate(segs):
            flat[b, :len(s)] = s
        count = np.array([len(s) for s in segs], np.int32)
        out = np.empty((B, H, W), np.uint8)
        self._check(self.lib.pd_op_draw_lines(self._h, flat.ctypes.data, count.ctypes.data, B, n, int(H), int(W), out.ctypes.data))
        return out

    def op_freeu_concat(self, h, skip, s: float, b: float, h_add=None, skip_add=None):
        """FreeU's skip concat of a decoder block (freeu_concat_kernel) in the residual-stream type: h, h_add [B, C_h, H, W];
        skip, skip_add [B or B/2, C_skip, H, W] -> [B, C_h + C_skip, H, W]."""
        f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        h, skip, h_add, skip_add = f(h), f(skip), f(h_add), f(skip_add)
        B, Ch, H, W = h.shape
        Cs = skip.shape[1]
        y = np.empty((B, Ch + Cs, H, W), np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.pd_op_freeu_concat(self._h, ptr(h), ptr(h_add), ptr(skip), ptr(skip_add), B, Ch, Cs, H, W,
                                                skip.shape[0], 0 if skip_add is None else skip_add.shape[0], float(s), float(b),
                                                y.ctypes.data))
        return y

    def op_sd3_update(self, shape, v=None, x=None, z0=None, mask=None, eps=None, use_cfg: bool = False, guidance: float = 1.0,
                      dsigma: float = 0.0, sigma: float = 0.0, pure: bool = False, seeded: bool = False, want_x_in: bool = False):
        """One launch of the SD3 loop's update kernel (pd_op_sd3_update) on [B, C, H, W] = shape, NumPy fp32.  v None: the start state
        from z0 / eps (or eps itself with pure); v [2B or B, C, H, W]: the CFG + Euler update of x by dsigma, blended with
        k = (1 - sigma) z0 + sigma eps under mask [B, 1, H, W].  seeded: eps is the engine's draw at ("xt", 0).  Returns the new
        state, and with want_x_in also the doubled input [2B, C, H, W] the kernel stores."""
        B, Cc, H, W = (int(s) for s in shape)
        f = lambda a, shp: None if a is None else np.ascontiguousarray(a, np.float32).reshape(shp)
        v = f(v, ((2 if use_cfg else 1) * B, Cc, H, W))
        x, z0, eps, mask = f(x, (B, Cc, H, W)), f(z0, (B, Cc, H, W)), f(eps, (B, Cc, H, W)), f(mask, (B, 1, H, W))
        ptr = lambda a: None if a is None else a.ctypes.data
        out = np.empty((B, Cc, H, W), np.float32)
        x_in = np.empty((2 * B, Cc, H, W), np.float32) if want_x_in else None
        self._check(self.lib.pd_op_sd3_update(self._h, ptr(v), ptr(x), ptr(z0), ptr(mask), ptr(eps), B, Cc, H, W, int(bool(use_cfg)),
                                              float(guidance), float(dsigma), float(sigma), int(bool(pure)), int(bool(seeded)), PD_MEM_HOST,
                                              ptr(out), ptr(x_in)))
        return (out, x_in) if want_x_in else out

    def op_ip_attention_add(self, q2, att, k_ip, v_ip, heads: int = 0, s: float = 1.0, scale: float = 0.0):
        """IP-Adapter's image term alone (ip_attn_add_kernel): att + s * softmax(q2 k_ip^T scale) v_ip per head in the compute type;
        q2, att [B, N, C]; k_ip, v_ip [B or 1, T, C]."""
        f = lambda a: np.ascontiguousarray(a, np.float32)
        q2, att, k_ip, v_ip = f(q2), f(att), f(k_ip), f(v_ip)
        B, N, Cc = q2.shape
        Bk, T, _ = k_ip.shape
        assert att.shape == q2.shape and v_ip.shape == k_ip.shape and k_ip.shape[2] == Cc
        out = np.empty_like(q2)
        self._check(self.lib.pd_op_ip_attention_add(self._h, q2.ctypes.data, att.ctypes.data, k_ip.ctypes.data, v_ip.ctypes.data, B, N, Cc,
                                                    int(heads), T, Bk, float(scale), float(s), out.ctypes.data))
        return out

    def op_spatial_transformer_ip(self, prefix: str, x, context, tokens):
        """op_spatial_transformer of a UNet block with the image term of tokens [B, T, context_dim] at the block's current scale."""
        x = np.ascontiguousarray(x, np.float32); ctx = np.ascontiguousarray(context, np.float32); tok = np.ascontiguousarray(tokens, np.float32)
        B, Cc, H, W = x.shape
        L = self._context_len(ctx, B, "context")
        assert tok.ndim == 3 and tok.shape[0] == B and tok.shape[2] == self.cfg.context_dim, tok.shape
        y = np.empty_like(x)
        self._check(self.lib.pd_op_spatial_transformer_ip(self._h, prefix.encode(), x.ctypes.data, ctx.ctypes.data, tok.ctypes.data, B, H, W, L,
                                                          int(tok.shape[1]), y.ctypes.data))
        return y

    def op_spatial_transformer(self, prefix: str, x, context):
        """SpatialTransformer.forward (attention.py:321-340) of the block loaded under `prefix`, through the sampling code path;
        context [B, L, context_dim] of any length L <= PD_MAX_CONTEXT_LEN."""
        x = np.ascontiguousarray(x, np.float32); ctx = np.ascontiguousarray(context, np.float32)
        B, Cc, H, W = x.shape
        L = self._context_len(ctx, B, "context")
        y = np.empty_like(x)
        self._check(self.lib.pd_op_spatial_transformer_ctx(self._h, prefix.encode(), x.ctypes.data, ctx.ctypes.data, B, H, W, L, y.ctypes.data))
        return y

    def bench_pag_identity(self, B: int, N: int, Cc: int, iters: int = 50) -> Tuple[float, float]:
        """(kernel ms, copy ms) per launch of pag_identity_kernel on [B, N, Cc] and of a device-to-device copy of the same bytes."""
        k, c = C.c_float(0), C.c_float(0)
        self._check(self.lib.pd_bench_pag_identity(self._h, int(B), int(N), int(Cc), int(iters), C.byref(k), C.byref(c)))
        return float(k.value), float(c.value)

    def op_pag_identity(self, vt, src: int, count: int):
        """pag_identity_kernel alone: vt [Bs, C, N] -> [count, N, C], samples [src, src + count) transposed, through the engine's storage type."""
        vt = np.ascontiguousarray(vt, np.float32)
        Bs, Cc, N = vt.shape
        out = np.empty((int(count), N, Cc), np.float32)
        self._check(self.lib.pd_op_pag_identity(self._h, vt.ctypes.data, Bs, Cc, N, int(src), int(count), out.ctypes.data))
        return out

    def op_cfg_combine(self, eps, B: int, use_cfg: bool, cfg_scale: float, pag_scale: float, eps_dtype: int = PD_DT_F32):
        """The guidance of the update kernel alone: eps [Bt, HW, C] = [uncond ;] cond [; perturbed] (the last only with pag_scale != 0),
        converted to eps_dtype on the device -> the guided eps [B, HW, C] fp32."""
        eps = np.ascontiguousarray(eps, np.float32)
        Bt, HW, Cc = eps.shape
        assert Bt == (2 if use_cfg else 1) * B + (B if pag_scale != 0 else 0), eps.shape
        out = np.empty((B, HW, Cc), np.float32)
        self._check(self.lib.pd_op_cfg_combine(self._h, eps.ctypes.data, int(B), HW, Cc, int(eps_dtype), int(bool(use_cfg)), float(cfg_scale),
                                               float(pag_scale), out.ctypes.data))
        return out

    def op_spatial_transformer_pag(self, prefix: str, x, context, n_perturbed: int):
        """op_spatial_transformer with the last n_perturbed samples perturbed: identity self-attention from their own V."""
        x = np.ascontiguousarray(x, np.float32); ctx = np.ascontiguousarray(context, np.float32)
        B, Cc, H, W = x.shape
        L = self._context_len(ctx, B, "context")
        y = np.empty_like(x)
        self._check(self.lib.pd_op_spatial_transformer_pag(self._h, prefix.encode(), x.ctypes.data, ctx.ctypes.data, B, H, W, L, int(n_perturbed),
                                                           y.ctypes.data))
        return y
