"""ctypes binding of libgdf.so (include/gdf.h) + `NativeUNet`, the MI355X-native stand-in for the
`pipe.unet` object that the reference calls at feature/diffusion_feature.py:445-465.

There is NO CPU / PyTorch fallback here on purpose: if the HIP library is missing or no GPU is
visible, construction raises.  PyTorch is only used for device memory, streams and tensor views.
"""
import collections
import ctypes as C
import math
import os
import time
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "libgdf.so")

GDF_F16, GDF_F32, GDF_BF16, GDF_BF16X2, GDF_FP8MX, GDF_F16S = 0, 1, 2, 3, 4, 5
MAX_LEVELS = 4


class ArchDesc(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("n_levels", C.c_int),
        ("block_out_channels", C.c_int * MAX_LEVELS), ("has_attn", C.c_int * MAX_LEVELS),
        ("transformer_layers", C.c_int * MAX_LEVELS), ("heads", C.c_int * MAX_LEVELS),
        ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int), ("use_linear_projection", C.c_int),
        ("time_embed_dim", C.c_int), ("addition_embed_text_time", C.c_int), ("addition_time_embed_dim", C.c_int),
        ("add_in_dim", C.c_int),
    ]


class PlanOpts(C.Structure):
    _fields_ = [("stream_fp32", C.c_int), ("early_exit", C.c_int), ("reserved", C.c_int * 6)]


class HookInfo(C.Structure):
    _fields_ = [("id", C.c_char_p), ("shape", C.c_int64 * 4), ("stride", C.c_int64 * 4), ("bytes", C.c_size_t)]


# symbol -> (restype, argtypes); every symbol declared in include/gdf.h
SIGNATURES = {
    "gdf_last_error": (C.c_char_p, []),
    "gdf_abi_version": (C.c_int, []),
    "gdf_model_create": (C.c_int, [C.POINTER(ArchDesc), C.POINTER(C.c_void_p)]),
    "gdf_model_destroy": (None, [C.c_void_p]),
    "gdf_model_param_count": (C.c_int, [C.c_void_p]),
    "gdf_model_param_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "gdf_model_param_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64 * 4)]),
    "gdf_model_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gdf_model_ready": (C.c_int, [C.c_void_p]),
    "gdf_model_weight_bytes": (C.c_size_t, [C.c_void_p]),
    "gdf_model_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "gdf_model_set_ready": (C.c_int, [C.c_void_p]),
    "gdf_model_hook_count": (C.c_int, [C.c_void_p]),
    "gdf_model_hook_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "gdf_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int,
                                  C.POINTER(PlanOpts), C.POINTER(C.c_void_p)]),
    "gdf_plan_destroy": (None, [C.c_void_p]),
    "gdf_plan_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "gdf_plan_num_ops": (C.c_int, [C.c_void_p]),
    "gdf_plan_hook_count": (C.c_int, [C.c_void_p]),
    "gdf_plan_hook_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(HookInfo)]),
    "gdf_plan_hook_copied": (C.c_int, [C.c_void_p, C.c_int]),
    "gdf_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_forward_res": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_plan_residual_count": (C.c_int, [C.c_void_p]),
    "gdf_plan_residual_bytes": (C.c_size_t, [C.c_void_p]),
    "gdf_plan_residual_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int64 * 4)]),
    "gdf_residual_count": (C.c_int, [C.POINTER(ArchDesc)]),
    "gdf_residual_bytes": (C.c_size_t, [C.POINTER(ArchDesc), C.c_int, C.c_int, C.c_int]),
    "gdf_residual_info": (C.c_int, [C.POINTER(ArchDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int64 * 4)]),
    "gdf_controlnet_create": (C.c_int, [C.POINTER(ArchDesc), C.POINTER(C.c_int * 4), C.c_int, C.POINTER(C.c_void_p)]),
    "gdf_controlnet_layout": (C.c_int, [C.POINTER(ArchDesc), C.POINTER(C.c_int * 4), C.c_int, C.POINTER(C.c_void_p)]),
    "gdf_controlnet_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PlanOpts), C.POINTER(C.c_void_p)]),
    "gdf_controlnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_controlnet_residual_bytes": (C.c_size_t, [C.c_void_p]),
    "gdf_plan_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int]),
    "gdf_trajectory": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_sample_state_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "gdf_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_op_guided_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "gdf_plan_set_graph": (C.c_int, [C.c_void_p, C.c_int]),
    "gdf_plan_graph_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "gdf_plan_graph_failures": (C.c_long, [C.c_void_p]),
    "gdf_plan_op_kernel": (C.c_char_p, [C.c_void_p, C.c_int]),
    "gdf_plan_num_kernel_labels": (C.c_int, [C.c_void_p]),
    "gdf_plan_kernel_label": (C.c_char_p, [C.c_void_p, C.c_int]),
    "gdf_plan_set_timing": (C.c_int, [C.c_void_p, C.c_char_p]),
    "gdf_plan_set_timing_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "gdf_plan_read_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "gdf_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gdf_stream_create_cu_mask": (C.c_int, [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_void_p)]),
    "gdf_stream_destroy": (C.c_int, [C.c_void_p]),
    "gdf_device_cu_count": (C.c_int, []),
    "gdf_cu_census": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
}



class FluxDesc(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("num_layers", C.c_int), ("num_single_layers", C.c_int),
                ("attention_head_dim", C.c_int), ("num_attention_heads", C.c_int), ("joint_attention_dim", C.c_int),
                ("pooled_projection_dim", C.c_int), ("guidance_embeds", C.c_int), ("axes_dims_rope", C.c_int * 3),
                ("mlp_ratio", C.c_int), ("compute_dtype", C.c_int)]


MAX_TIMESTEPS = 8                    # GDF_MAX_TIMESTEPS (include/gdf.h; tests/test_multi_t_cpu.py holds the two together)


class VaeDesc(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("latent_channels", C.c_int), ("n_levels", C.c_int),
                ("block_out_channels", C.c_int * MAX_LEVELS), ("layers_per_block", C.c_int), ("use_quant_conv", C.c_int)]


# every symbol declared in include/gdf_vae.h
SIGNATURES.update({
    "gdf_vae_model_create": (C.c_int, [C.POINTER(VaeDesc), C.POINTER(C.c_void_p)]),
    "gdf_vae_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "gdf_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_vae_encode_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_vae_plan_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_double), C.c_int]),
    "gdf_vae_encode_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
})

# the decoder half of include/gdf_vae.h (`vae-out`)
SIGNATURES.update({
    "gdf_vae_decoder_create": (C.c_int, [C.POINTER(VaeDesc), C.POINTER(C.c_void_p)]),
    "gdf_vae_decode_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "gdf_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_vae_decode_plan_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int]),
})


class PixartDesc(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("num_attention_heads", "attention_head_dim", "in_channels", "out_channels", "num_layers",
                                       "patch_size", "sample_size", "caption_channels", "interpolation_scale")]


# every symbol declared in include/gdf_pixart.h
SIGNATURES.update({
    "gdf_pixart_model_create": (C.c_int, [C.POINTER(PixartDesc), C.POINTER(C.c_void_p)]),
    "gdf_pixart_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int,
                                         C.POINTER(PlanOpts), C.POINTER(C.c_void_p)]),
    "gdf_pixart_forward": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_pixart_plan_profile": (C.c_int, [C.c_void_p] * 5 + [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int]),
})

# every symbol declared in include/gdf_flux.h
SIGNATURES.update({
    "gdf_flux_model_create": (C.c_int, [C.POINTER(FluxDesc), C.POINTER(C.c_void_p)]),
    "gdf_flux_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int,
                                       C.POINTER(PlanOpts), C.POINTER(C.c_void_p)]),
    "gdf_flux_forward": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gdf_flux_plan_profile": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int]),
})

# the kernel-level entries of include/gdf_ops.h that the package itself calls (SIGNATURES stays the model-level headers' table): the device
# Canny (csrc/canny.hip) and the device image preprocessing (csrc/preproc.hip)
GDF_CANNY_U8_HWC3, GDF_CANNY_U8_HW, GDF_CANNY_F32_NCHW, GDF_CANNY_F16_NCHW = 0, 1, 2, 3
GDF_CANNY_DST_U8, GDF_CANNY_DST_F16_NCHW3 = 0, 1
OP_SIGNATURES = {
    "gdf_op_canny_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "gdf_op_canny_classify": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gdf_op_canny_link": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gdf_op_canny": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # the device PIL-to-tensor step (csrc/preproc.hip; components/preproc.py calls it)
    "gdf_op_pil_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "gdf_op_pil_resize_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "gdf_op_pil_resize_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None

# operand-plan levels, the plan chooser and the verify ladder live in components/plan_levels.py (round 6); re-exported here for the callers
# that import them from this module
from .plan_levels import (AUTO_BOUND, AUTO_BOUND_BY_FAMILY, RES_EXPONENT, SELECTIVE_BY_ARCH, SPLIT_ALL, SPLIT_CLASSES, SPLIT_DEEP_EXTRA,  # noqa: F401
                          SPLIT_LIGHT, SPLIT_SELECTIVE, VerifyLadder, arch_family, auto_bound, choose_split, split_mask, table_scale)


def make_cu_partition_streams(dev, parts=2, layout="interleave"):
    """`parts` HIP streams restricted to disjoint, equal sets of CUs of `dev` (hipExtStreamCreateWithCUMask through
    gdf_stream_create_cu_mask) -> ([torch.cuda.ExternalStream], CUs per partition).
    layout "interleave": CU i belongs to partition i % parts; "block": contiguous ranges of the mask."""
    lib = load_library()
    with torch.cuda.device(dev):
        n = lib.gdf_device_cu_count()
        if n <= 0 or n % (8 * parts):
            raise RuntimeError(f"cannot split {n} CUs into {parts} partitions of a multiple of 8")
        per = n // parts
        out = []
        for k in range(parts):
            words = (C.c_uint32 * ((n + 31) // 32))()
            for i in range(n):
                if (i % parts == k) if layout == "interleave" else (i // per == k):
                    words[i // 32] |= (1 << (i % 32))
            h = C.c_void_p()
            _check(lib.gdf_stream_create_cu_mask(words, len(words), C.byref(h)), "stream_create_cu_mask")
            out.append(torch.cuda.ExternalStream(h.value, device=dev))
    return out, per


def lib_path():
    return _LIB_PATH


def load_library():
    """dlopen libgdf.so and bind every symbol of include/gdf.h. Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(OP_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError => header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        msg = load_library().gdf_last_error()
        raise RuntimeError(f"libgdf {what} failed (status {rc}): {msg.decode() if msg else ''}")


def _create(fn, what):
    """Model creation = one hipMalloc of the weight arena OUTSIDE torch's caching allocator.  When that fails for lack of memory the memory is
    usually there — as blocks torch has cached (freed tensors it keeps for reuse; a long-lived process that builds and drops extractors piles
    them up: tools/soak.py saw 280 GB cached on a 288-GB device) — so: collect, hand torch's cache back to the driver, try once more."""
    rc = fn()
    if rc != 0:
        msg = (load_library().gdf_last_error() or b"").decode()
        if "out of memory" in msg or "hipMalloc" in msg:
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            rc = fn()
    _check(rc, what)


def canny(src, low=100, high=200, out='control'):
    """cv2.Canny(image, low, high) on the device (gdf_op_canny, csrc/canny.hip), queued on the CURRENT stream; nothing is read back.
    src: a tensor on a HIP device — uint8 (B, H, W, 3) (np.array of RGB PIL images) or (B, H, W), or fp32 / fp16 (B, 3, H, W) in [-1, 1], which is
    quantised as the reference's restore_from_tensor_to_image does: preprocess_image's tensor gives the bytes it was made from.
    out: 'control' -> fp16 (B, 3, H, W) of 0.0 / 1.0, what control_tensor makes of the reference's three-channel edge image and what
    NativeControlNet.forward_raw(cond=) takes; 'u8' -> uint8 (B, H, W) of 0 / 255, cv2's output.
    The workspace is an ordinary allocation of the caller's stream pool, freed (stream-ordered) on return.  There is no CPU fallback."""
    if not (torch.is_tensor(src) and src.is_cuda):
        raise RuntimeError("canny: the source must be a tensor on a HIP device; there is no CPU fallback")
    if out not in ('control', 'u8'):
        raise ValueError("canny: out is 'control' or 'u8'")
    if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[-1] == 3:
        kind, (B, H, W) = GDF_CANNY_U8_HWC3, src.shape[:3]
    elif src.dtype == torch.uint8 and src.dim() == 3:
        kind, (B, H, W) = GDF_CANNY_U8_HW, src.shape
    elif src.dtype in (torch.float32, torch.float16) and src.dim() == 4 and src.shape[1] == 3:
        kind, (B, _, H, W) = (GDF_CANNY_F32_NCHW if src.dtype == torch.float32 else GDF_CANNY_F16_NCHW), src.shape
    else:
        raise ValueError(f"canny: uint8 (B, H, W, 3) or (B, H, W), or fp32 / fp16 (B, 3, H, W); got {src.dtype} {tuple(src.shape)}")
    lib = load_library()
    src = src.contiguous()
    dev = src.device
    with torch.cuda.device(dev):
        nbytes = lib.gdf_op_canny_workspace_bytes(B, H, W)
        if nbytes == 0:
            raise ValueError(f"canny: {B} x {H} x {W} is empty or has 2^31 pixels or more (32-bit component labels)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = (torch.empty((B, 3, H, W), dtype=torch.float16, device=dev) if out == 'control'
               else torch.empty((B, H, W), dtype=torch.uint8, device=dev))
        _check(lib.gdf_op_canny(C.c_void_p(src.data_ptr()), kind, B, H, W, math.floor(low), math.floor(high), C.c_void_p(dst.data_ptr()),
                                GDF_CANNY_DST_F16_NCHW3 if out == 'control' else GDF_CANNY_DST_U8, C.c_void_p(ws.data_ptr()),
                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "op_canny")
    return dst


# --------------------------------------------------------------------------------------------- #
# architecture descriptors: the UNet `config.json` fields the reference reads via diffusers
# (components/models.py:18-56 of the reference select the HF repos these come from)
# --------------------------------------------------------------------------------------------- #
ARCH_CONFIGS = {
    "1-5": dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
                has_attn=(1, 1, 1, 0), transformer_layers=(1, 1, 1, 1), heads=(8, 8, 8, 8), layers_per_block=2,
                cross_attention_dim=768, use_linear_projection=0, time_embed_dim=1280, addition_embed_text_time=0,
                addition_time_embed_dim=0, add_in_dim=0),
    "xl": dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280),
               has_attn=(0, 1, 1), transformer_layers=(1, 2, 10), heads=(5, 10, 20), layers_per_block=2,
               cross_attention_dim=2048, use_linear_projection=1, time_embed_dim=1280, addition_embed_text_time=1,
               addition_time_embed_dim=256, add_in_dim=2816),
}
ARCH_CONFIGS["pgv2"] = ARCH_CONFIGS["xl"]        # Playground-v2 shares the SDXL UNet architecture
# SD 2.1-base (reference models.py:30-42): the SD1.5 topology with 64-wide heads (5, 10, 20, 20), OpenCLIP-H text width 1024
# and linear proj_in / proj_out (config.json of stabilityai/stable-diffusion-2-1-base)
ARCH_CONFIGS["2-1"] = dict(ARCH_CONFIGS["1-5"], heads=(5, 10, 20, 20), cross_attention_dim=1024, use_linear_projection=1)


def arch_desc(cfg):
    a = ArchDesc()
    n = len(cfg["block_out_channels"])
    a.in_channels, a.out_channels, a.n_levels = cfg["in_channels"], cfg["out_channels"], n
    for i in range(n):
        a.block_out_channels[i] = cfg["block_out_channels"][i]
        a.has_attn[i] = int(cfg["has_attn"][i])
        a.transformer_layers[i] = cfg["transformer_layers"][i]
        a.heads[i] = cfg["heads"][i]
    a.layers_per_block = cfg["layers_per_block"]
    a.cross_attention_dim = cfg["cross_attention_dim"]
    a.use_linear_projection = int(cfg["use_linear_projection"])
    a.time_embed_dim = cfg["time_embed_dim"]
    a.addition_embed_text_time = int(cfg["addition_embed_text_time"])
    a.addition_time_embed_dim = cfg["addition_time_embed_dim"]
    a.add_in_dim = cfg["add_in_dim"]
    return a


def residual_layout(cfg, batch, lat_h, lat_w):
    """The ControlNet residual block of architecture `cfg` at (batch, lat_h, lat_w) (include/gdf.h, gdf_forward_res) ->
    ([(byte offset, (B, C, H, W))] with the mid block's tensor last, bytes of the block).  Host arithmetic: needs the library, no GPU."""
    lib = load_library()
    a = arch_desc(cfg)
    out = []
    for i in range(lib.gdf_residual_count(C.byref(a))):
        off, shape = C.c_size_t(), (C.c_int64 * 4)()
        _check(lib.gdf_residual_info(C.byref(a), batch, lat_h, lat_w, i, C.byref(off), C.byref(shape)), "residual_info")
        out.append((off.value, tuple(shape)))
    return out, lib.gdf_residual_bytes(C.byref(a), batch, lat_h, lat_w)


def config_from_diffusers(uc):
    """Map a diffusers UNet2DConditionModel.config (or a raw config.json namespace: fields the constructor defaults are read with
    those defaults) onto ARCH_CONFIGS fields."""
    boc = tuple(uc.block_out_channels)
    n = len(boc)
    tl = getattr(uc, "transformer_layers_per_block", 1)
    tl = tuple(tl) if isinstance(tl, (list, tuple)) else (tl,) * n
    ahd = uc.attention_head_dim
    ahd = tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * n
    text_time = getattr(uc, "addition_embed_type", None) == "text_time"
    return dict(in_channels=uc.in_channels, out_channels=getattr(uc, "out_channels", uc.in_channels), block_out_channels=boc,
                has_attn=tuple(int("CrossAttn" in t) for t in uc.down_block_types), transformer_layers=tl, heads=ahd,
                layers_per_block=getattr(uc, "layers_per_block", 2), cross_attention_dim=uc.cross_attention_dim,
                use_linear_projection=int(bool(getattr(uc, "use_linear_projection", False))), time_embed_dim=boc[0] * 4,
                addition_embed_text_time=int(text_time),
                addition_time_embed_dim=(getattr(uc, "addition_time_embed_dim", None) or 0) if text_time else 0,
                add_in_dim=(getattr(uc, "projection_class_embeddings_input_dim", None) or 0) if text_time else 0)


class _Lease:
    """One hand-out of a hook-buffer set.  The tensors a forward returns are views of ONE tensor created from this object through the CUDA
    array interface, so their shared storage keeps the lease alive; when the caller has dropped every view (and every view of a view), the
    storage dies, the lease's finalizer runs and the set may be handed out again.  Public API only (round 3 used the private
    torch._C._storage_Use_Count for this liveness test)."""

    def __init__(self, ptr, n_halves):
        self.__cuda_array_interface__ = dict(shape=(n_halves,), typestr="<f2", data=(ptr, False), version=2)


_SETS_BY_PTR = {}            # base device pointer of a hook-buffer set -> weakref to its _HookSet (release_after's lookup)
import threading as _threading
_SETS_LOCK = _threading.Lock()   # one extractor per host thread is a supported mode (reference aggregation_network.py:67-95)


def _forget_set(lo):
    """weakref.finalize callback of a _HookSet: drop its entry (unless a NEW set already lives at that address)"""
    with _SETS_LOCK:
        r = _SETS_BY_PTR.get(lo)
        if r is not None and r() is None:
            del _SETS_BY_PTR[lo]


def release_after(tensors, stream=None):
    """Tell the library that hook tensors returned by a forward / FeatureExtractor.extract are still being READ on `stream` (default: the
    current stream) by work queued so far — the analogue of Tensor.record_stream() for these buffers.  The buffers are recycled (and then
    overwritten by a later forward) once the caller has dropped every reference; work on the stream that was current at extract() time is
    ordered automatically, a consumer on ANY OTHER stream calls this after queueing its reads and may then drop the tensors at once.
    `tensors`: a tensor, a dict of tensors (the extract() result) or an iterable of tensors.
    Returns the CUDA tensors that are NOT backed by a hook-buffer set (caching-allocator tensors such as pooled / aggregated features):
    the caller protects those the ordinary way, `t.record_stream(stream)`."""
    if torch.is_tensor(tensors):
        tensors = [tensors]
    elif isinstance(tensors, dict):
        tensors = list(tensors.values())
    done = set()
    unmatched = []
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            continue
        p = t.untyped_storage().data_ptr()       # every view of a hand-out shares the lease tensor's storage, which starts at the set's base
        with _SETS_LOCK:
            ref = _SETS_BY_PTR.get(p)
        hs = ref() if ref is not None else None
        if hs is None:
            unmatched.append(t)
            continue
        if id(hs) in done:
            continue
        done.add(id(hs))
        s = stream if stream is not None else torch.cuda.current_stream(t.device)
        ev = torch.cuda.Event()
        ev.record(s)
        hs.events.append(ev)
        # a one-off / evicted set may die before it is handed out again: then its allocation goes back to the caching allocator, which
        # must not hand the memory to the plan's stream while `s` still reads it
        hs.buf.record_stream(s)
    return unmatched


class _HookSet:
    """One set of caller-visible output buffers of a plan (every hook + the model output) carved out of ONE allocation.
    The tensors a forward returns are views of a per-hand-out lease tensor over it (`_Lease`); the set may be handed out again only when
    the caller has dropped every such view, so returned dicts stay valid for as long as they are referenced (reference contract:
    FeatureStore.reset() rebinds a fresh dict, feature_extractor.py:28-29).
    Reuse is STREAM-ORDERED: the next forward runs on the plan's stream after `side.wait_stream(current)` AND after every event
    registered through release_after() — so work the caller queued on its current stream, or announced on another stream, is ordered
    before the buffers are overwritten, and the host keeps queueing forwards without waiting for the GPU."""

    def __init__(self, plan, out_elems, dev):
        import weakref
        self.offs, tot = [], 0
        for (_, _, _, nbytes) in plan.hooks:
            self.offs.append(tot)
            tot += (nbytes // 2 + 127) // 128 * 128
        self.out_off = tot
        tot += (out_elems + 127) // 128 * 128
        self.n = max(tot, 128)
        self.buf = torch.empty(self.n, dtype=torch.float16, device=dev)      # owned by the set for its whole life; never handed out itself
        base = self.buf.data_ptr()
        self.lo, self.hi = base, base + 2 * self.n
        self.ptrs = (C.c_void_p * max(1, len(self.offs)))(*[base + 2 * o for o in self.offs])
        self.out_ptr = C.c_void_p(base + 2 * self.out_off)
        self.leased = False
        self.events = []                 # release_after(): reads still in flight on other streams
        with _SETS_LOCK:
            _SETS_BY_PTR[self.lo] = weakref.ref(self)
        weakref.finalize(self, _forget_set, self.lo)           # no unbounded registry in processes that never call release_after

    def lease(self, dev):
        """-> fp16 tensor over the whole set whose storage keeps the lease alive; the set is free again when that storage dies"""
        import weakref
        le = _Lease(self.lo, self.n)
        le._owner = self                 # a one-off set (not pooled by its plan) lives exactly as long as its views
        self.leased = True
        me = weakref.ref(self)

        def _released(me=me):
            hs = me()
            if hs is not None:
                hs.leased = False
        weakref.finalize(le, _released)
        with torch.cuda.device(dev):
            return torch.as_tensor(le, device=dev)

    def free(self):
        return not self.leased


class _Plan:
    """A libgdf plan + everything with a STABLE device address it runs on: workspace, input staging buffers, up to MAX_SETS
    hook-buffer sets and a private non-default stream.  Stable addresses are what lets gdf_plan_set_graph replay one recorded
    hipGraph per set instead of rebuilding it (the graph cache of the library is keyed on the buffer addresses)."""
    MAX_SETS = 3
    # Forwards queued ahead of the GPU (GDF_MAX_INFLIGHT, 0 = unbounded = the default).  With many forwards queued the AQL ring fills
    # and the launching thread SPINS inside hipGraphLaunch (BENCH_r02: 35 ms of host CPU per 114-ms step with 20 steps queued; 0.4 ms
    # with 5).  Round 3 measured the alternatives on the same box (bench.py `hipgraph.host_cpu_ms_per_step`, 20 steps): a bound of 2 with
    # a blocking-sync event.synchronize() 204 ms (every wait of this runtime spins, also with hipDeviceScheduleBlockingSync:
    # tools/micro/sync_cpu.py), a bound of 2 with a 0.5-ms sleep-poll on event.query() 102 ms (a runtime helper thread spins while
    # the event is polled), unbounded 35 ms — identical throughput (141.6 / 141.9 img/s).  So the queue stays unbounded; the knob
    # remains for hosts that prefer a shallow queue.
    # Round 5: in a multi-rank job (WORLD_SIZE > 1) the default is 4 — eight spinning launch threads are eight burnt cores, and the
    # sleep-poll bound costs ~0.4 ms of host CPU per step at unchanged throughput.
    MAX_INFLIGHT = int(os.environ.get("GDF_MAX_INFLIGHT", "4" if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 else "0"))

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle
        self.graph = os.environ.get("GDF_HIP_GRAPH", "1") not in ("", "0")   # hipGraph replay (gdf.h)
        lib.gdf_plan_set_graph(handle, int(self.graph))
        self.ws_bytes = lib.gdf_plan_workspace_bytes(handle)
        self.hooks = []
        for i in range(lib.gdf_plan_hook_count(handle)):
            hi = HookInfo()
            _check(lib.gdf_plan_hook_info(handle, i, C.byref(hi)), "plan_hook_info")
            self.hooks.append((hi.id.decode(), tuple(hi.shape), tuple(hi.stride), hi.bytes))
        self.workspace = None
        self.stream = None               # a torch.cuda.ExternalStream over a stream of this plan's own (gdf_stream_create), or one assigned by the caller
        self._own_stream = None          # its hipStream_t when this plan created it
        self.staged = {}
        self.sets = []
        self.inflight = []
        self.out_capacity = 0            # elements every set's output region holds at least (a plan whose calls differ in output size sets it ONCE,
                                         # before its first run: NativeVAEEncoder._plan)

    def __del__(self):
        # The plan's buffers (workspace, staging, hook sets) are ordinary allocations of the CALLER's stream pool that only this plan's stream
        # writes: its queued work ends before they go back to that pool (and before the stream goes away).
        try:
            if self.stream is not None:
                self.stream.synchronize()
        except Exception:
            pass
        try:
            self.lib.gdf_plan_destroy(self.handle)
        except Exception:
            pass
        self.workspace = None
        self.staged = {}
        self.sets = []
        try:
            if self._own_stream is not None:
                self.lib.gdf_stream_destroy(self._own_stream)
        except Exception:
            pass

    def _make_stream(self, dev):
        """a non-blocking stream owned by this plan — never torch's pooled streams, which are shared by every 32nd request (include/gdf.h)"""
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _check(self.lib.gdf_stream_create(C.byref(h)), "stream_create")
        self._own_stream = h
        return torch.cuda.ExternalStream(h.value, device=dev)

    def graph_stats(self):
        """(graphs built, graph launches, forwards that fell back to eager launching after a failed construction / instantiation)"""
        cap, lau = C.c_long(), C.c_long()
        self.lib.gdf_plan_graph_stats(self.handle, C.byref(cap), C.byref(lau))
        return cap.value, lau.value, int(self.lib.gdf_plan_graph_failures(self.handle))

    def _stage_buffer(self, name, t, dtype, dev, side):
        """the persistent staging buffer of input `name` (allocated on the caller's stream: see run)"""
        if t is None:
            return None
        b = self.staged.get(name)
        if b is None or b.shape != t.shape or b.dtype != dtype:
            if b is not None:
                side.synchronize()
            b = self.staged[name] = torch.empty(t.shape, dtype=dtype, device=dev)
        return b

    def _stage(self, name, t, dtype, dev):
        """copy `t` into the persistent staging buffer of input `name` (dtype conversion + layout in the same copy)"""
        if t is None:
            return None
        b = self.staged[name]
        b.copy_(t, non_blocking=True)
        return b

    def run(self, dev, inputs, out_shape, call, profile=False, eager=False, out_dtype=torch.float16):
        """Stage `inputs` [(name, tensor | None, dtype)], pick a free hook-buffer set and launch `call(staged, hook_ptrs,
        out_ptr, ws_ptr, stream_ptr)` on the plan's private stream, event-ordered after the caller's current stream; the
        caller's stream then waits for it, so results follow ordinary stream semantics.
        Returns (out tensor, {hook id: (B,C,H,W) view}, whatever `call` returned)."""
        cur = torch.cuda.current_stream(dev)
        if self.stream is None:
            self.stream = self._make_stream(dev)
        side = self.stream
        while self.MAX_INFLIGHT > 0 and len(self.inflight) >= self.MAX_INFLIGHT:
            ev = self.inflight.pop(0)
            while not ev.query():                  # sleep-poll: hipEventSynchronize / hipStreamSynchronize SPIN on this runtime even with
                time.sleep(0.0005)                 # blocking-sync events or hipDeviceScheduleBlockingSync (tools/micro/sync_cpu.py:
                                                   # 48 ms of CPU per 48 ms of waiting; the poll: 0.3 ms)
        n_out = 1
        for d in out_shape:
            n_out *= d
        # Allocations happen HERE, on the caller's stream — i.e. in the pool every other allocation of the process uses — not under the plan's
        # private stream: torch caches freed blocks per stream, a plan's stream dies with the plan, and blocks cached for a dead stream are never
        # handed out again (tools/soak.py: ~800 extractor lifetimes filled 288 GB with such blocks).  Only this plan's stream writes them, and
        # only behind the side.wait_stream(cur) BELOW: a block this allocation reuses may have been freed a moment ago with reads still queued on
        # `cur` (by any thread — the default stream is shared), and the wait is what orders those reads before the plan's first write.
        # __del__ drains the plan's stream before the blocks are returned.
        with torch.cuda.device(dev):
            if self.workspace is None or self.workspace.numel() < self.ws_bytes:
                if self.workspace is not None:
                    side.synchronize()                          # (a smaller one may still be in use by queued work)
                self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
            for (n, t, dt) in inputs:
                self._stage_buffer(n, t, dt, dev, side)
            hs = next((h for h in self.sets if h.free()), None)
            pooled = True
            if hs is None:
                hs = _HookSet(self, max(n_out, self.out_capacity), dev)
                pooled = len(self.sets) < self.MAX_SETS        # more live result sets than that: one-off buffers, run eagerly
                if pooled:
                    self.sets.append(hs)
                # (a one-off set dies with its last view, possibly while this forward still runs: its block then returns to `cur`'s pool, and
                #  whatever is allocated from it next is written by work queued on `cur` behind the cur.wait_stream(side) below)
        side.wait_stream(cur)
        with torch.cuda.device(dev), torch.cuda.stream(side):
            staged = [self._stage(n, t, dt, dev) for (n, t, dt) in inputs]
            for ev in hs.events:                               # readers announced through release_after(): ordered before the overwrite
                side.wait_event(ev)
            hs.events = []
            no_graph = self.graph and (eager or profile or not pooled)
            if no_graph:
                self.lib.gdf_plan_set_graph(self.handle, 0)
            try:
                ret = call(staged, hs.ptrs, hs.out_ptr, C.c_void_p(self.workspace.data_ptr()), C.c_void_p(side.cuda_stream))
            finally:
                if no_graph:
                    self.lib.gdf_plan_set_graph(self.handle, 1)
            if self.MAX_INFLIGHT > 0:
                done = torch.cuda.Event()
                done.record(side)
                self.inflight.append(done)
        cur.wait_stream(side)
        base = hs.lease(dev)                                   # every returned tensor is a view of this one hand-out (see _Lease)
        feats = {}
        for off, (hid, shape, stride, _) in zip(hs.offs, self.hooks):
            feats[hid] = torch.as_strided(base, shape, stride, storage_offset=off)
        out = base[hs.out_off:hs.out_off + n_out].view(out_dtype).view(out_shape)      # fp16 or bf16: same 16-bit container
        return out, feats, ret


_T_CACHE = {}


def _timestep_on_device(timestep, B, dev):
    """(B,) float32 device tensor of the timestep(s).  A HOST timestep (number / CPU tensor: what FeatureExtractor passes since round 5) is
    looked up in a small cache of device constants — a pageable host -> device copy is stream ordered and would block the host until the
    previous forward has finished; a device tensor is used as it is."""
    if torch.is_tensor(timestep) and timestep.is_cuda:
        t = timestep.to(dev).float().reshape(-1)
        return t.expand(B) if t.numel() == 1 else t
    vals = tuple(float(v) for v in torch.as_tensor(timestep).reshape(-1).tolist())
    key = (vals, B, str(dev))
    t = _T_CACHE.get(key)
    if t is None:
        if len(_T_CACHE) > 256:
            _T_CACHE.clear()
        t = torch.tensor(vals, dtype=torch.float32, device=dev)
        t = _T_CACHE[key] = (t.expand(B) if t.numel() == 1 else t).contiguous()
    return t


class _NativeModel:
    """Shared surface of the libgdf model wrappers: weights in / hook names out (include/gdf.h model functions)."""
    _arena_fp16 = True       # weight matrices live as fp16 images in the device arena (the MMDiT keeps bf16 / its own cast report: NativeFluxTransformer)

    lib = None
    handle = None
    device = None
    split = 0          # split-operand classes of the plans (UNet only; see NativeUNet)

    def _is_norm(self, name):
        """True for norm parameters (synthetic init: weight 1 + 0.1 N, bias 0.1 N)."""
        return False

    # ---- nn.Module-like surface used by FeatureExtractor -------------------------------------
    def parameters(self):
        return iter(())

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def __del__(self):
        try:
            self._plans.clear()
            self.lib.gdf_model_destroy(self.handle)
        except Exception:
            pass

    # ---- weights ----------------------------------------------------------------------------------
    def param_shapes(self):
        out = {}
        for i in range(self.lib.gdf_model_param_count(self.handle)):
            shp = (C.c_int64 * 4)()
            nd = self.lib.gdf_model_param_shape(self.handle, i, C.byref(shp))
            out[self.lib.gdf_model_param_name(self.handle, i).decode()] = tuple(shp[:nd])
        return out

    def hook_names(self):
        return [self.lib.gdf_model_hook_name(self.handle, i).decode()
                for i in range(self.lib.gdf_model_hook_count(self.handle))]

    def load_state_dict(self, sd, strict=True):
        """sd: diffusers UNet2DConditionModel state_dict (name -> tensor, any device, fp16/fp32)."""
        shapes = self.param_shapes()
        missing = [k for k in shapes if k not in sd]
        if strict and missing:
            raise KeyError(f"missing UNet parameters: {missing[:5]} ... ({len(missing)})")
        stream = torch.cuda.current_stream(self.device)
        inexact = torch.zeros((), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for name, shp in shapes.items():
                if name not in sd:
                    continue
                t = sd[name]
                if tuple(t.shape) != shp:
                    raise ValueError(f"{name}: expected shape {shp}, got {tuple(t.shape)}")
                if t.dtype not in (torch.float16, torch.float32, torch.bfloat16):
                    t = t.float()
                t = t.to(self.device, non_blocking=True).contiguous()
                if self._arena_fp16 and t.dtype != torch.float16 and t.dim() >= 2:       # (norm / bias vectors stay fp32 in the arena)
                    inexact += (t.half().to(t.dtype) != t).any()
                code = {torch.float16: GDF_F16, torch.float32: GDF_F32, torch.bfloat16: GDF_BF16}[t.dtype]
                _check(self.lib.gdf_model_set_param(self.handle, name.encode(), C.c_void_p(t.data_ptr()), code,
                                                    C.c_void_p(stream.cuda_stream)), f"set_param({name})")
                del t
            stream.synchronize()
        # The MFMA operands are 16-bit: a weight matrix is ONE fp16 image in the arena (the split plans pair the ACTIVATIONS, not the weights).
        # A checkpoint whose matrices are not fp16-exact (dtype='float32' pipelines: reference feature/components/models.py:11-12) is therefore
        # the fp16-rounded checkpoint — the very weights the reference's own dtype='float16' mode computes with — and sits ~1e-3 from the
        # fp32-weight model whatever the operand plan (tests/test_gpu_diffusers_branch.py test_float32_dtype_real_checkpoint_branch).
        self.weights_rounded = int(inexact) > 0
        if self.weights_rounded:
            import warnings
            warnings.warn(f"gdf {type(self).__name__}: {int(inexact)} weight matrices of this checkpoint are not exactly representable in fp16 and were "
                          "rounded once at load (the native models keep fp16 weight images): the features are those of the fp16-rounded checkpoint — what "
                          "dtype='float16' loads — about 1e-3 (relative L2) from the fp32-weight model", RuntimeWarning, stacklevel=2)
        return self

    def init_synthetic(self, seed=0, chunk_elems=1 << 26):
        """Seeded synthetic weights generated directly in HBM (no checkpoints exist offline):
        W ~ N(0, 1/fan_in), bias ~ 0.05 N, norm gamma = 1 + 0.1 N, beta = 0.1 N (fp16-rounded)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            for name, shp in self.param_shapes().items():
                is_norm = self._is_norm(name)
                t = torch.randn(shp, generator=g, device=self.device, dtype=torch.float32)
                if name.endswith(".weight") and not is_norm:
                    fan_in = 1
                    for s in shp[1:]:
                        fan_in *= s
                    t.mul_(fan_in ** -0.5)
                elif name.endswith(".weight"):
                    t.mul_(0.1).add_(1.0)
                elif is_norm:
                    t.mul_(0.1)
                else:
                    t.mul_(0.05)
                t = t.half()
                _check(self.lib.gdf_model_set_param(self.handle, name.encode(), C.c_void_p(t.data_ptr()), GDF_F16,
                                                    C.c_void_p(stream.cuda_stream)), f"set_param({name})")
                stream.synchronize()
        return self

    def ready(self):
        return bool(self.lib.gdf_model_ready(self.handle))

    def weight_blob(self):
        """The device weight arena as a flat uint8 tensor (zero-copy view; include/gdf.h gdf_model_weights)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        _check(self.lib.gdf_model_weights(self.handle, C.byref(ptr), C.byref(n)), "model_weights")
        holder = types.SimpleNamespace(__cuda_array_interface__=dict(shape=(n.value,), typestr="|u1", data=(ptr.value, False),
                                                                     version=2), _owner=self)
        with torch.cuda.device(self.device):
            return torch.as_tensor(holder, device=self.device)

    def set_ready(self):
        _check(self.lib.gdf_model_set_ready(self.handle), "model_set_ready")
        return self

    def _launch(self, plan, fwd, prof_fn, what, profile):
        """-> call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr) for _Plan.run; `args(staged)` orders the staged inputs"""
        lib = self.lib

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            head = [plan.handle] + [vp(a) for a in staged]
            if not profile:
                _check(fwd(*head, hook_ptrs, out_ptr, ws_ptr, stream_ptr), what)
                return None
            n = lib.gdf_plan_num_ops(plan.handle)
            ms = (C.c_float * n)(); names = (C.c_char_p * n)(); fl = (C.c_double * n)()
            if prof_fn(*head, hook_ptrs, out_ptr, ws_ptr, stream_ptr, ms, names, fl, n) < 0:
                _check(1, what + " (profile)")
            return [(names[i].decode(), ms[i], fl[i], lib.gdf_plan_op_kernel(plan.handle, i).decode()) for i in range(n)]
        return call

    def requested_ids(self):
        fs = self.feature_store
        if fs is None:
            return []
        if fs.accept_all:
            return self.hook_names()
        return [k for k, v in fs.to_store.items() if v]


class NativeUNet(_NativeModel):
    """UNet2DConditionModel replacement running entirely in libgdf.so (hand-written HIP, gfx950).

    Call signature mirrors the reference's use at feature/diffusion_feature.py:446-465:
        unet(latent_model_input, timestep=t, encoder_hidden_states=prompt_embeds,
             added_cond_kwargs={...}, down_block_additional_residuals=None,
             mid_block_additional_residual=None, return_dict=False)[0]
    Hooked activations are delivered to `self.feature_store` (components/feature_extractor.py) in
    execution order, as (B,C,H,W)-shaped fp16 tensors stored channels-last.
    """

    def __init__(self, cfg, device="cuda", stream_fp32=True, early_exit=False, precise=None, verify=None):
        """verify=True (or GDF_VERIFY=1): runtime self-check of the automatic plan level — see _verify_level.
        precise=True (or GDF_PRECISE=1): opt-in split-operand plans — every activation operand of a GEMM / conv and every
        GroupNorm input is kept as an fp16 pair hi + lo and multiplied as [hi | lo] x [W | W] (include/gdf.h, gdf_plan_opts):
        removes the fp16-operand rounding that bounds the default plans at 1.0-1.3e-3 on `ffn-inner` / `unet-out`; every hook
        then meets the 1e-3 target of BASELINE.json at about twice the GEMM time."""
        if not torch.cuda.is_available():
            raise RuntimeError("NativeUNet needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg)
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self._arch = arch_desc(cfg)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_model_create(C.byref(self._arch), C.byref(h)), "model_create")
        self.handle = h
        self.stream_fp32 = bool(stream_fp32)
        self.early_exit = bool(early_exit)
        # split-operand classes of the plans: `precise` = None / 'auto' (default: chosen per hook set, choose_split) | False (plain fp16
        # operands) | True | 'selective' | 'stream,attn_out' | mask.  GDF_PRECISE in the environment supplies the default.
        env = os.environ.get("GDF_PRECISE")
        self.set_precise(precise if precise is not None else (env if env not in (None, "") else "auto"))
        self.last_split = 0
        # runtime self-check of the 'auto' plan level: the chooser's table is a CPU emulation on synthetic N(0, 1/fan_in)
        # weights; real checkpoints have heavy-tailed statistics.  With verify on, the FIRST forward of every hook set also runs the full
        # split and compares the requested hooks; a level whose worst hook differs by more than VERIFY_BOUND is escalated (plain -> selective
        # -> full) for that hook set from then on, with one warning.
        self.verify = (os.environ.get("GDF_VERIFY", "0") not in ("", "0")) if verify is None else bool(verify)
        self._ladder = VerifyLadder(self.cfg)    # escalations found, layer sets verified, log, acceptance bound (components/plan_levels.py)
        self.cus = 0                     # > 0: plans are sized for a CU partition of that many CUs and run on `self.partition_stream`
        self.partition_stream = None     # torch.cuda.ExternalStream over a CU-masked HIP stream (make_cu_partition_streams)
        self.feature_store = None
        self.shared_ctx = False          # set by FeatureExtractor.extract (it repeats one prompt over the batch)
        self.extra_hook_ids = []         # hooks FeatureExtractor needs internally (aggregated `attention=` feature)
        self.last_extra = {}
        self._plans = {}
        self.dtype = torch.float16
        # attributes the reference reads from pipe.unet (diffusion_feature.py:544-547)
        self.config = types.SimpleNamespace(
            in_channels=cfg["in_channels"], addition_time_embed_dim=cfg["addition_time_embed_dim"],
            sample_size=None, cross_attention_dim=cfg["cross_attention_dim"])
        self.add_embedding = types.SimpleNamespace(linear_1=types.SimpleNamespace(in_features=cfg["add_in_dim"]))

    @property
    def precise(self):
        """True when the plans keep EVERY operand class split (the round-3 `precise` plans)"""
        return (not getattr(self, "auto_split", False)) and self.split == SPLIT_ALL

    @precise.setter
    def precise(self, v):
        self.set_precise(v)

    def set_precise(self, spec):
        """'auto': the cheapest plan level that keeps every REQUESTED hook within 1e-3 (choose_split); anything else: split_mask(spec)"""
        self.auto_split = isinstance(spec, str) and spec.strip().lower() == "auto"
        self.split = 0 if self.auto_split else split_mask(spec)
        return self

    def split_for(self, hook_ids, lat=None):
        if getattr(self, "auto_split", False):
            # (split plans need the fp32 master of the stream: the opt-out fp16-stream mode keeps plain operands)
            if not self.stream_fp32:
                return 0
            return self._ladder.split_for(hook_ids, lat)
        return self.split

    def _verify_level(self, run, ids, out):
        """The runtime self-check behind verify=True / GDF_VERIFY=1: components/plan_levels.py VerifyLadder.check decides; this method binds it to
        the plans — the level kept becomes `last_split`, and every plan of THIS layer set at another level (the full split's, the rungs tried and
        rejected, the table's own choice when it was escalated) goes away with its workspace and hook sets."""
        key = tuple(ids)
        try:
            out, kept = self._ladder.check(run, ids, out, self.last_split)
        finally:
            keep = self._ladder.escalated.get(key, self.last_split) if key in self._ladder.verified else self.last_split
            self._drop_plans({k for k in self._plans if k[4] == key and k[8] != keep})
        self.last_split = kept
        return out

    # (the ladder's state under the names tests and tools have used since round 4)
    verify_log = property(lambda self: self._ladder.log)
    _verified = property(lambda self: self._ladder.verified)
    _escalated = property(lambda self: self._ladder.escalated)
    verify_bound = property(lambda self: self._ladder.bound_override, lambda self, v: setattr(self._ladder, "bound_override", v))
    FULL_SPLIT_ERROR = VerifyLadder.FULL_SPLIT_ERROR

    def verify_accept_bound(self):
        return self._ladder.accept_bound()

    def _drop_plans(self, keys):
        for k in keys:
            self._plans.pop(k, None)

    def _is_norm(self, name):
        return ".norm" in name or name.startswith("conv_norm_out")

    # ---- plans ------------------------------------------------------------------------------------
    def _plan(self, batch, h, w, n_ctx, hook_ids, shared_ctx=False, split=None, early_exit=None, residuals=False):
        split = self.split_for(hook_ids, lat=min(h, w)) if split is None else split
        early_exit = self.early_exit if early_exit is None else bool(early_exit)
        key = (batch, h, w, n_ctx, tuple(hook_ids), self.stream_fp32, early_exit, bool(shared_ctx), split, self.cus, bool(residuals))
        p = self._plans.get(key)
        if p is None:
            ids = (C.c_char_p * max(1, len(hook_ids)))(*[s.encode() for s in hook_ids])
            opts = PlanOpts(int(self.stream_fp32), int(early_exit))
            opts.reserved[0] = int(bool(shared_ctx))
            opts.reserved[1] = 1 if split == SPLIT_ALL else (split << 8)
            opts.reserved[2] = int(self.cus)
            opts.reserved[3] = int(bool(residuals))
            ph = C.c_void_p()
            _check(self.lib.gdf_plan_create(self.handle, batch, h, w, n_ctx, ids, len(hook_ids), C.byref(opts),
                                            C.byref(ph)), "plan_create")
            p = _Plan(self.lib, ph)
            if self.partition_stream is not None:
                p.stream = self.partition_stream
            if len(self._plans) >= 8:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    # ---- forward ------------------------------------------------------------------------------------
    def forward_raw(self, sample, timestep, encoder_hidden_states, text_embeds=None, time_ids=None, hook_ids=None,
                    profile=False, shared_ctx=False, residuals=None):
        """Returns (noise_pred (B,4,H,W) view, OrderedDict id -> hook tensor). Inputs must live on self.device.
        shared_ctx=True promises that every row-block of encoder_hidden_states equals the first one (one prompt repeated
        over the batch, as FeatureExtractor.extract does): the text K/V projections are then computed once per call.
        residuals: the ControlNet residual block (gdf_forward_res, include/gdf.h): a flat fp16 device tensor of
        residual_layout(B, H, W)[1] bytes laid out as that function says (pack_residuals builds one from NCHW tensors)."""
        dev = self.device
        B, _, H, W = sample.shape
        if residuals is not None:
            if profile:
                raise NotImplementedError("per-op profiling of a forward with residuals: time its kernel with gdf_plan_set_timing instead")
            need = self.residual_layout(B, H, W)[1]
            if residuals.dtype != torch.float16 or residuals.dim() != 1 or residuals.numel() * 2 != need:
                raise ValueError(f"the residual block must be a flat fp16 tensor of {need} bytes for batch {B}, latent {H}x{W}")
        ctx = encoder_hidden_states
        t = _timestep_on_device(timestep, B, dev)
        txt = tid = None
        if self.cfg["addition_embed_text_time"]:
            if text_embeds is None or time_ids is None:
                raise ValueError("added_cond_kwargs with text_embeds and time_ids is required for this UNet")
            txt, tid = text_embeds, time_ids
            pooled = self.cfg["add_in_dim"] - 6 * self.cfg["addition_time_embed_dim"]
            if tuple(txt.shape) != (B, pooled) or tuple(tid.shape) != (B, 6):
                raise ValueError(f"text_embeds {tuple(txt.shape)} / time_ids {tuple(tid.shape)} do not match the model "
                                 f"(expected ({B},{pooled}) / ({B},6))")
        if ctx.shape[0] != B or ctx.shape[2] != self.cfg["cross_attention_dim"]:
            raise ValueError("encoder_hidden_states shape mismatch")
        ids = list(hook_ids) if hook_ids is not None else self.requested_ids()
        self.last_split = self.split_for(ids, lat=min(H, W))
        has_res = residuals is not None
        plan = self._plan(B, H, W, ctx.shape[1], ids, shared_ctx, self.last_split, residuals=has_res)
        f16, f32 = torch.float16, torch.float32
        fwd = self.lib.gdf_forward_res if has_res else self.lib.gdf_forward
        inputs = [("sample", sample, f16), ("t", t, f32), ("ctx", ctx, f16), ("txt", txt, f16), ("tid", tid, f32)]
        if has_res:
            inputs.append(("res", residuals, f16))        # (staged like every input: a stable address for the plan's graph)
        call = self._launch(plan, fwd, self.lib.gdf_plan_profile, "forward", profile)
        noise, out, prof = plan.run(dev, inputs, (B, H, W, self.cfg["out_channels"]), call, profile=profile)
        noise_nchw = noise.permute(0, 3, 1, 2)
        if profile:
            return noise_nchw, out, prof
        if self.verify and getattr(self, "auto_split", False) and self.stream_fp32 and tuple(ids) not in self._verified:
            def run(mask):
                pl = self._plan(B, H, W, ctx.shape[1], ids, shared_ctx, mask, residuals=has_res)    # (every level sees the same residual block)
                cl = self._launch(pl, fwd, self.lib.gdf_plan_profile, "forward", False)
                n_, o_, _ = pl.run(dev, inputs, (B, H, W, self.cfg["out_channels"]), cl)
                return n_.permute(0, 3, 1, 2), o_
            noise_nchw, out = self._verify_level(run, ids, (noise_nchw, out))
        return noise_nchw, out

    # ---- multi-step latent trajectory ---------------------------------------------------------------------
    TRAJECTORY_MAX_STEPS = 1024          # GDF_TRAJECTORY_MAX_STEPS (include/gdf.h)

    def trajectory(self, latents_f32, table, encoder_hidden_states, text_embeds=None, time_ids=None, shared_ctx=False, eager=False):
        """len(table) x (one hook-less forward + one scheduler update) on the device (gdf_trajectory, include/gdf.h): row k of `table` is
        (timestep, c_in, c_sample, c_eps); forward k sees fp16(c_in[k] * x_k) at timestep[k], then x_{k+1} = c_sample[k] x_k + c_eps[k] noise_pred_k
        on the fp32 master.  Returns the final fp32 latents (B,4,H,W) as a new tensor; `latents_f32` is not modified.
        The plan has no hooks (the reference pauses its feature store meanwhile, diffusion_feature.py:384-386).  Its operand-split level is the
        one the CURRENT feature selection (requested_ids) gives the extraction forward that consumes the result: the latents are that forward's
        input and are not computed at a coarser level than its hooks are promised at."""
        dev = self.device
        B, _, H, W = latents_f32.shape
        ctx = encoder_hidden_states
        rows = [tuple(float(v) for v in r) for r in table]
        if not rows or len(rows) > self.TRAJECTORY_MAX_STEPS or any(len(r) != 4 for r in rows):
            raise ValueError(f"table must hold 1..{self.TRAJECTORY_MAX_STEPS} rows of (timestep, c_in, c_sample, c_eps)")
        txt = tid = None
        if self.cfg["addition_embed_text_time"]:
            if text_embeds is None or time_ids is None:
                raise ValueError("text_embeds and time_ids are required for this UNet")
            txt, tid = text_embeds, time_ids
            pooled = self.cfg["add_in_dim"] - 6 * self.cfg["addition_time_embed_dim"]
            if tuple(txt.shape) != (B, pooled) or tuple(tid.shape) != (B, 6):
                raise ValueError(f"text_embeds {tuple(txt.shape)} / time_ids {tuple(tid.shape)} do not match the model "
                                 f"(expected ({B},{pooled}) / ({B},6))")
        if ctx.shape[0] != B or ctx.shape[2] != self.cfg["cross_attention_dim"]:
            raise ValueError("encoder_hidden_states shape mismatch")
        ids = self.requested_ids()
        have = set(ids)
        split = self.split_for(ids + [i for i in self.extra_hook_ids if i not in have], lat=min(H, W))
        plan = self._plan(B, H, W, ctx.shape[1], (), shared_ctx, split, early_exit=False)
        flat = (C.c_float * (4 * len(rows)))(*[v for r in rows for v in r])
        lib = self.lib

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            x32, c, tx, ti = staged
            _check(lib.gdf_trajectory(plan.handle, vp(x32), len(rows), flat, vp(c), vp(tx), vp(ti), out_ptr, ws_ptr, stream_ptr), "trajectory")

        f16, f32 = torch.float16, torch.float32
        plan.run(dev, [("x32", latents_f32, f32), ("ctx", ctx, f16), ("txt", txt, f16), ("tid", tid, f32)],
                 (B, H, W, self.cfg["out_channels"]), call, eager=eager)
        # the master lives in the plan's staging buffer, which the next call overwrites: hand out a copy (ordered on the caller's stream)
        return plan.staged["x32"].clone()

    # ---- guided sampling with hook capture at selected UNet calls -------------------------------------------------
    def sample(self, latents_f32, rows, guidance, ctx_pos, ctx_neg=None, text_embeds=None, time_ids=None, hook_ids=(), capture_rows=(),
               eager=False):
        """len(rows) x (one forward + one guided scheduler update) on the device (gdf_sample, include/gdf.h).  Row k of `rows` is
        (timestep, c_in, c_sample, w0, w1, w2, w3, w4) (components/models.py sampling_table): forward k sees fp16(c_in[k] * x_k) at timestep[k],
        then e_k = e_uncond + guidance (e_cond - e_uncond) and x_{k+1} = c_sample[k] x_k + sum_j w_j[k] e_{k-j} on the fp32 master.
        guidance > 1: the forwards have batch 2B, [ctx_neg, ctx_pos] (torch.cat([negative, positive])), and `text_embeds` / `time_ids`
        already hold both halves in that order (2B rows).  guidance <= 1: batch B, ctx_pos alone, as diffusers does.
        The rows listed in `capture_rows` run a plan with `hook_ids` instead of the hook-less one.
        Returns (final fp32 latents (B,4,H,W), a new tensor; {row: OrderedDict id -> (2B|B, C, H, W) fp16}).
        Both plans run at ONE operand-split level, chosen the way `trajectory` chooses it: the level the requested hooks (hook_ids plus the
        current feature selection) are promised at.  The call BYPASSES the verify ladder (`verify=True` checks single forwards only)."""
        dev = self.device
        B, _, H, W = latents_f32.shape
        guided = float(guidance) > 1.0
        table = [tuple(float(v) for v in r) for r in rows]
        if not table or len(table) > self.TRAJECTORY_MAX_STEPS or any(len(r) != 8 for r in table):
            raise ValueError(f"rows must hold 1..{self.TRAJECTORY_MAX_STEPS} rows of (timestep, c_in, c_sample, w0, w1, w2, w3, w4)")
        caps = [int(k) for k in capture_rows]
        if any(k < 0 or k >= len(table) for k in caps) or any(b <= a for a, b in zip(caps, caps[1:])):
            raise ValueError("capture_rows must be ascending row indices of `rows`")
        hook_ids = list(hook_ids)
        if caps and not hook_ids:
            raise ValueError("capture_rows without hook_ids")
        if guided:
            if ctx_neg is None or ctx_neg.shape != ctx_pos.shape:
                raise ValueError("a guided run needs ctx_neg of ctx_pos's shape")
            ctx = torch.cat([ctx_neg.to(dev), ctx_pos.to(dev)], 0)
        else:
            ctx = ctx_pos.to(dev)
        PB = 2 * B if guided else B
        txt = tid = None
        if self.cfg["addition_embed_text_time"]:
            if text_embeds is None or time_ids is None:
                raise ValueError("text_embeds and time_ids are required for this UNet")
            txt, tid = text_embeds, time_ids
            pooled = self.cfg["add_in_dim"] - 6 * self.cfg["addition_time_embed_dim"]
            if tuple(txt.shape) != (PB, pooled) or tuple(tid.shape) != (PB, 6):
                raise ValueError(f"text_embeds {tuple(txt.shape)} / time_ids {tuple(tid.shape)} do not match the model "
                                 f"(expected ({PB},{pooled}) / ({PB},6))")
        if ctx.shape[0] != PB or ctx.shape[2] != self.cfg["cross_attention_dim"]:
            raise ValueError("encoder_hidden_states shape mismatch")
        have = set(hook_ids)
        promised = hook_ids + [i for i in self.requested_ids() + list(self.extra_hook_ids) if i not in have]
        split = self.split_for(promised, lat=min(H, W))
        plain = self._plan(PB, H, W, ctx.shape[1], (), False, split, early_exit=False)
        hooked = self._plan(PB, H, W, ctx.shape[1], hook_ids, False, split, early_exit=False) if caps else None
        lib = self.lib
        flat = (C.c_float * (8 * len(table)))(*[v for r in table for v in r])
        cap_arr = (C.c_int * max(1, len(caps)))(*caps)
        f16, f32 = torch.float16, torch.float32
        # Buffers of this call (allocated on the caller's stream, written on the plain plan's: _Plan.run orders the two).  The state block
        # and the hooked plan's workspace keep their addresses from call to call, so the graphs keep theirs; the capture buffers are new
        # tensors that belong to the caller.
        with torch.cuda.device(dev):
            nst = int(lib.gdf_sample_state_bytes(PB, H, W, len(table)))
            st = getattr(plain, "sample_state", None)
            if st is None or st.numel() < nst:
                if st is not None and plain.stream is not None:
                    plain.stream.synchronize()
                st = plain.sample_state = torch.empty(nst, dtype=torch.uint8, device=dev)
            captured, ptrs = {}, []
            ws_h = None
            if hooked is not None:
                if hooked.workspace is None or hooked.workspace.numel() < hooked.ws_bytes:
                    hooked.workspace = torch.empty(hooked.ws_bytes, dtype=torch.uint8, device=dev)
                ws_h = hooked.workspace
                offs, tot = [], 0
                for (_, _, _, nbytes) in hooked.hooks:
                    offs.append(tot)
                    tot += (nbytes // 2 + 127) // 128 * 128
                for k in caps:
                    buf = torch.empty(max(tot, 128), dtype=f16, device=dev)
                    od = collections.OrderedDict()
                    for off, (hid, shape, stride, _) in zip(offs, hooked.hooks):
                        od[hid] = torch.as_strided(buf, shape, stride, storage_offset=off)
                        ptrs.append(buf.data_ptr() + 2 * off)
                    captured[k] = od
            hook_arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            x32, c, tx, ti = staged
            # Capture rows run eagerly: every call brings new hook buffers, and a graph is keyed on them (one build per capture and call
            # otherwise).  Their launches are queued while the GPU is still busy with the replayed rows before them.
            off = hooked is not None and hooked.graph                        # (the plain plan's switch is _Plan.run's)
            if off:
                lib.gdf_plan_set_graph(hooked.handle, 0)
            try:
                _check(lib.gdf_sample(plain.handle, hooked.handle if hooked is not None else None, vp(x32), len(table), flat,
                                      C.c_float(float(guidance)), vp(c), vp(tx), vp(ti), cap_arr, len(caps), hook_arr, out_ptr, vp(st), ws_ptr,
                                      vp(ws_h), stream_ptr), "sample")
            finally:
                if off:
                    lib.gdf_plan_set_graph(hooked.handle, 1)

        plain.run(dev, [("x32", latents_f32, f32), ("ctx", ctx, f16), ("txt", txt, f16), ("tid", tid, f32)],
                  (PB, H, W, self.cfg["out_channels"]), call, eager=eager)
        # the master lives in the plan's staging buffer, which the next call overwrites: hand out a copy (ordered on the caller's stream)
        return plain.staged["x32"].clone(), captured

    # ---- ControlNet residuals ---------------------------------------------------------------------------
    def residual_layout(self, batch, lat_h, lat_w):
        """([(byte offset, (B, C, H, W))], bytes) of the residual block of this UNet (module-level residual_layout)"""
        return residual_layout(self.cfg, batch, lat_h, lat_w)

    def residual_buffer(self, batch, lat_h, lat_w, n_ctx, hook_ids=None, shared_ctx=False):
        """The staged residual block of the plan forward_raw(residuals=...) will pick for these arguments: a flat fp16 tensor with a stable
        address.  A producer that writes it in place (NativeControlNet.forward_raw(out=...)) and hands the same tensor to forward_raw saves
        the staging copy; handing any other tensor (or reaching another plan) is as correct and costs that copy."""
        ids = list(hook_ids) if hook_ids is not None else self.requested_ids()
        plan = self._plan(batch, lat_h, lat_w, n_ctx, ids, shared_ctx, self.split_for(ids, lat=min(lat_h, lat_w)), residuals=True)
        n = self.residual_layout(batch, lat_h, lat_w)[1] // 2
        b = plan.staged.get("res")
        if b is None or b.numel() != n:
            if b is not None and plan.stream is not None:
                plan.stream.synchronize()
            with torch.cuda.device(self.device):
                b = plan.staged["res"] = torch.empty(n, dtype=torch.float16, device=self.device)
        return b

    def pack_residuals(self, down_block_additional_residuals, mid_block_additional_residual):
        """Torch (B, C, H, W) residuals of any ControlNet -> the flat fp16 block forward_raw takes (channels-last tensors at the offsets of
        residual_layout).  ValueError on a wrong count or shape."""
        down = list(down_block_additional_residuals)
        mid = mid_block_additional_residual
        if mid.dim() != 4:
            raise ValueError(f"mid_block_additional_residual must be (B, C, H, W), got {tuple(mid.shape)}")
        B = mid.shape[0]
        n = self.cfg["layers_per_block"] * len(self.cfg["block_out_channels"]) + len(self.cfg["block_out_channels"])
        if len(down) != n:
            raise ValueError(f"down_block_additional_residuals has {len(down)} tensors, this UNet has {n} skips")
        up = 1 << (len(self.cfg["block_out_channels"]) - 1)
        lay, nbytes = self.residual_layout(B, mid.shape[2] * up, mid.shape[3] * up)
        block = torch.zeros(nbytes // 2, dtype=torch.float16, device=self.device)
        for i, (t, (off, shape)) in enumerate(zip(down + [mid], lay)):
            if tuple(t.shape) != shape:
                raise ValueError(f"{'mid residual' if i == n else 'down residual %d' % i} has shape {tuple(t.shape)}, expected {shape}")
            b, c, h, w = shape
            block[off // 2:off // 2 + b * c * h * w].view(b, h, w, c).copy_(t.permute(0, 2, 3, 1))
        return block

    def __call__(self, sample, timestep=None, encoder_hidden_states=None, added_cond_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict=False,
                 **kwargs):
        residuals = None
        if down_block_additional_residuals is not None and mid_block_additional_residual is not None:    # `is_controlnet`, unet_2d_condition.py:1194
            residuals = self.pack_residuals(down_block_additional_residuals, mid_block_additional_residual)
            if residuals.numel() * 2 != self.residual_layout(*[sample.shape[i] for i in (0, 2, 3)])[1]:
                raise ValueError("the residuals do not match the sample's batch and latent size")
        elif down_block_additional_residuals is not None:
            raise NotImplementedError("down_block_additional_residuals without mid_block_additional_residual is the deprecated T2I-Adapter "
                                      "route of the reference (unet_2d_condition.py:1200-1210): not on the native path")
        elif mid_block_additional_residual is not None:
            raise ValueError("mid_block_additional_residual needs down_block_additional_residuals (unet_2d_condition.py:1194)")
        akw = added_cond_kwargs or {}
        ids = self.requested_ids()
        have = set(ids)
        ids = ids + [i for i in self.extra_hook_ids if i not in have]
        noise, hooks = self.forward_raw(sample, timestep, encoder_hidden_states, akw.get("text_embeds"),
                                        akw.get("time_ids"), hook_ids=ids, shared_ctx=self.shared_ctx, residuals=residuals)
        self.last_extra = {k: v for k, v in hooks.items() if k in set(self.extra_hook_ids)}
        if self.feature_store is not None:
            for hid, t in hooks.items():
                if hid in have:
                    self.feature_store.store(t, hid)
        if return_dict:
            return types.SimpleNamespace(sample=noise)
        return (noise,)


# --------------------------------------------------------------------------------------------- #
# ControlNet (include/gdf_control.h): diffusers' ControlNetModel over the encoder half of a UNet architecture
# (reference components/controlnet.py:95-130)
# --------------------------------------------------------------------------------------------- #
COND_CHANNELS = (16, 32, 96, 256)        # conditioning_embedding_out_channels of every checkpoint the reference loads


def controlnet_param_shapes(cfg, cond_channels=COND_CHANNELS, conditioning_channels=3):
    """{name: shape} of a ControlNetModel state dict over architecture `cfg`, in libgdf's registration order (host arithmetic: no GPU)"""
    lib = load_library()
    a, cc, h = arch_desc(cfg), (C.c_int * 4)(*cond_channels), C.c_void_p()
    _check(lib.gdf_controlnet_layout(C.byref(a), C.byref(cc), conditioning_channels, C.byref(h)), "controlnet_layout")
    try:
        out = {}
        for i in range(lib.gdf_model_param_count(h)):
            shp = (C.c_int64 * 4)()
            nd = lib.gdf_model_param_shape(h, i, C.byref(shp))
            out[lib.gdf_model_param_name(h, i).decode()] = tuple(shp[:nd])
        return out
    finally:
        lib.gdf_model_destroy(h)


class NativeControlNet(_NativeModel):
    """ControlNetModel replacement running entirely in libgdf.so: the conditioning embedding (csrc/cond_embed.hip), the UNet's down and mid
    program, and one 1x1 conv per skip written straight into the residual block NativeUNet.forward_raw(residuals=...) reads."""

    def __init__(self, cfg, device="cuda", cond_channels=COND_CHANNELS, conditioning_channels=3, stream_fp32=True):
        if not torch.cuda.is_available():
            raise RuntimeError("NativeControlNet needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg)
        self.cond_channels = tuple(int(c) for c in cond_channels)
        self.conditioning_channels = int(conditioning_channels)
        if len(self.cond_channels) != 4:
            raise ValueError("conditioning_embedding_out_channels must have four entries")
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self._arch = arch_desc(cfg)
        h = C.c_void_p()
        cc = (C.c_int * 4)(*self.cond_channels)
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_controlnet_create(C.byref(self._arch), C.byref(cc), self.conditioning_channels, C.byref(h)),
                    "controlnet_create")
        self.handle = h
        self.stream_fp32 = bool(stream_fp32)
        self.feature_store = None
        self._plans = {}
        self.dtype = torch.float16
        self.config = types.SimpleNamespace(conditioning_embedding_out_channels=self.cond_channels, conditioning_channels=self.conditioning_channels,
                                            global_pool_conditions=False, cross_attention_dim=cfg["cross_attention_dim"])

    def _is_norm(self, name):
        return ".norm" in name

    def residual_layout(self, batch, lat_h, lat_w):
        return residual_layout(self.cfg, batch, lat_h, lat_w)

    def _plan(self, batch, h, w, n_ctx, shared_ctx=False, split=0, direct=False):
        """direct: the plan of the calls that write into a caller's block (out=); its result sets hold no block of their own"""
        key = (batch, h, w, n_ctx, self.stream_fp32, bool(shared_ctx), split, bool(direct))
        p = self._plans.get(key)
        if p is None:
            opts = PlanOpts(int(self.stream_fp32), 0)
            opts.reserved[0] = int(bool(shared_ctx))
            opts.reserved[1] = 1 if split == SPLIT_ALL else (split << 8)
            ph = C.c_void_p()
            _check(self.lib.gdf_controlnet_plan_create(self.handle, batch, h, w, n_ctx, C.byref(opts), C.byref(ph)), "controlnet_plan_create")
            p = _Plan(self.lib, ph)
            if len(self._plans) >= 8:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def forward_raw(self, sample, timestep, encoder_hidden_states, text_embeds=None, time_ids=None, cond=None, shared_ctx=False, split=0,
                    out=None, eager=False):
        """-> the residual block: a flat fp16 tensor of residual_layout(B, H, W)[1] bytes (skips in diffusers' order, the mid block's last).
        cond: the control image (B, conditioning_channels, 8 H, 8 W) in [0, 1], fp16 or fp32.  shared_ctx / split: as NativeUNet's plans
        (split: a mask of SPLIT_CLASSES).  out: a flat fp16 device tensor of that size — the plan writes straight into it and it is returned."""
        dev = self.device
        B, _, H, W = sample.shape
        if cond is None or cond.dim() != 4 or tuple(cond.shape) != (B, self.conditioning_channels, 8 * H, 8 * W):
            raise ValueError(f"controlnet_cond must be ({B}, {self.conditioning_channels}, {8 * H}, {8 * W}), got "
                             f"{None if cond is None else tuple(cond.shape)}")
        if cond.dtype not in (torch.float16, torch.float32):
            cond = cond.float()
        ctx = encoder_hidden_states
        t = _timestep_on_device(timestep, B, dev)
        txt = tid = None
        if self.cfg["addition_embed_text_time"]:
            if text_embeds is None or time_ids is None:
                raise ValueError("added_cond_kwargs with text_embeds and time_ids is required for this ControlNet")
            txt, tid = text_embeds, time_ids
            pooled = self.cfg["add_in_dim"] - 6 * self.cfg["addition_time_embed_dim"]
            if tuple(txt.shape) != (B, pooled) or tuple(tid.shape) != (B, 6):
                raise ValueError(f"text_embeds {tuple(txt.shape)} / time_ids {tuple(tid.shape)} do not match the model "
                                 f"(expected ({B},{pooled}) / ({B},6))")
        if ctx.shape[0] != B or ctx.shape[2] != self.cfg["cross_attention_dim"]:
            raise ValueError("encoder_hidden_states shape mismatch")
        need = self.residual_layout(B, H, W)[1]
        if out is not None and (out.dtype != torch.float16 or out.dim() != 1 or out.numel() * 2 != need or not out.is_contiguous()
                                or out.device != dev or out.data_ptr() % 256):
            raise ValueError(f"out must be a flat, 256-byte aligned fp16 tensor of {need} bytes on {dev}")
        plan = self._plan(B, H, W, ctx.shape[1], shared_ctx, int(split), direct=out is not None)
        f16, f32 = torch.float16, torch.float32
        inputs = [("sample", sample, f16), ("t", t, f32), ("ctx", ctx, f16), ("txt", txt, f16), ("tid", tid, f32), ("cond", cond, cond.dtype)]
        code = GDF_F32 if cond.dtype == f32 else GDF_F16
        lib = self.lib

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            dst = C.c_void_p(out.data_ptr()) if out is not None else out_ptr
            _check(lib.gdf_controlnet_forward(plan.handle, *[vp(a) for a in staged], code, dst, ws_ptr, stream_ptr), "controlnet_forward")
        block, _, _ = plan.run(dev, inputs, (128,) if out is not None else (need // 2,), call, eager=eager)
        return out if out is not None else block

    def views(self, block, batch, lat_h, lat_w):
        """-> ([NCHW views of the skips' residuals], NCHW view of the mid block's) of a flat block"""
        v = [block[off // 2:off // 2 + b * c * h * w].view(b, h, w, c).permute(0, 3, 1, 2)
             for off, (b, c, h, w) in self.residual_layout(batch, lat_h, lat_w)[0]]
        return v[:-1], v[-1]

    def __call__(self, sample, timestep=None, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0, guess_mode=False,
                 added_cond_kwargs=None, return_dict=False, **kwargs):
        if conditioning_scale != 1 or guess_mode:
            raise NotImplementedError("the native ControlNet runs conditioning_scale = 1, guess_mode = False (what the reference's extraction uses)")
        akw = added_cond_kwargs or {}
        block = self.forward_raw(sample, timestep, encoder_hidden_states, akw.get("text_embeds"), akw.get("time_ids"), controlnet_cond)
        down, mid = self.views(block, sample.shape[0], sample.shape[2], sample.shape[3])
        if return_dict:
            return types.SimpleNamespace(down_block_res_samples=down, mid_block_res_sample=mid)
        return down, mid


def native_controlnet_from(module, device="cuda"):
    """A NativeControlNet from any object with diffusers' ControlNetModel surface: `.config` and `.state_dict()`."""
    c = module.config
    if getattr(c, "global_pool_conditions", False):
        raise ValueError("global_pool_conditions is not supported by the native ControlNet")
    if getattr(c, "controlnet_conditioning_channel_order", "rgb") != "rgb":
        raise ValueError("controlnet_conditioning_channel_order must be 'rgb'")
    if getattr(c, "class_embed_type", None) is not None:
        raise ValueError("class_embed_type is not supported by the native ControlNet")
    cn = NativeControlNet(config_from_diffusers(c), device, tuple(getattr(c, "conditioning_embedding_out_channels", COND_CHANNELS)),
                          getattr(c, "conditioning_channels", 3))
    return cn.load_state_dict({k: v for k, v in module.state_dict().items()})


# --------------------------------------------------------------------------------------------- #
# MMDiT / Flux (include/gdf_flux.h): FluxTransformer2DModel `config.json` of black-forest-labs/FLUX.1-dev
# (reference components/models.py:150-169)
# --------------------------------------------------------------------------------------------- #
FLUX_CONFIGS = {
    "flux": dict(in_channels=64, num_layers=19, num_single_layers=38, attention_head_dim=128, num_attention_heads=24,
                 joint_attention_dim=4096, pooled_projection_dim=768, guidance_embeds=1, axes_dims_rope=(16, 56, 56),
                 mlp_ratio=4),
}


def flux_desc(cfg):
    d = FluxDesc()
    for k in ("in_channels", "num_layers", "num_single_layers", "attention_head_dim", "num_attention_heads",
              "joint_attention_dim", "pooled_projection_dim"):
        setattr(d, k, int(cfg[k]))
    d.guidance_embeds = int(bool(cfg["guidance_embeds"]))
    d.mlp_ratio = int(cfg.get("mlp_ratio", 4))
    d.compute_dtype = {"bfloat16": GDF_BF16, "float16": GDF_F16, "bfloat16x2": GDF_BF16X2, "fp8-mx": GDF_FP8MX, "float16s": GDF_F16S,
                       "auto": GDF_F16S}[cfg.get("compute_dtype", "bfloat16")]
    for i in range(3):
        d.axes_dims_rope[i] = int(cfg["axes_dims_rope"][i])
    return d


class SingleForwardDone(Exception):
    """Raised by NativeFluxTransformer.__call__ (single_forward=True) after its first forward of a pipeline call; carries the
    model output.  See FeatureExtractor.extract (flux branch)."""

    def __init__(self, sample):
        super().__init__("single denoiser forward done")
        self.sample = sample


class NativeFluxTransformer(_NativeModel):
    """FluxTransformer2DModel replacement running entirely in libgdf.so (hand-written HIP, gfx950).

    Call signature mirrors the pipeline's use of `self.transformer(...)` (FluxImg2ImgPipeline, invoked by the reference
    at feature/diffusion_feature.py:246-254) == FluxTransformer2DModel.forward
    (feature/diffusers/models/transformers/transformer_flux.py:414-428):
        transformer(hidden_states=latents, timestep=t/1000, guidance=g, pooled_projections=..., encoder_hidden_states=...,
                    txt_ids=..., img_ids=..., joint_attention_kwargs=None, return_dict=False)[0]
    Hooked activations go to `self.feature_store` in execution order as (B, C, h, w) fp16 tensors (channels-last),
    ids `vit-block{i}-{q,k,v,attn-out,norm-out,ffn-inner,out}` (components/feature_extractor.py:98-123).
    """
    _arena_fp16 = False

    FP16_CAST_TOL = 1e-4       # 'auto': relative Frobenius error a weight matrix may lose in the bf16 -> fp16 cast before the mode falls back

    def __init__(self, cfg, device="cuda", early_exit=False, compute_dtype=None):
        """compute_dtype:
          "bfloat16"   what the reference loads Flux in (components/models.py:158-169); hooks <= 3.4e-3 of the fp32 reference at full depth
          "float16"    3 more mantissa bits, plain fp16 range on every 16-bit tensor (<= 4.6e-4)
          "float16s"   float16 with the MLP hidden tensors range-scaled by 2^-8 (include/gdf_flux.h GDF_F16S): same accuracy and speed, no
                       operand class left whose range is not bounded a priori or by the reference's own fp16 hooks
          "auto"       (the product default, components/models.py) = "float16s" guarded at load time: every weight matrix must survive the
                       bf16 -> fp16 cast (FP16_CAST_TOL); a checkpoint that does not is loaded as "bfloat16x2" instead, with one warning
          "bfloat16x2" bf16 hi + lo operand pairs (<= 1.8e-4, bf16's range everywhere, ~1.65x the time)
          "fp8-mx"     opt-in e4m3 MFMA leg, LOWER precision (<= 7.5e-2)."""
        if not torch.cuda.is_available():
            raise RuntimeError("NativeFluxTransformer needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg)
        if compute_dtype is not None:
            self.cfg["compute_dtype"] = compute_dtype
        self.cfg.setdefault("compute_dtype", "bfloat16")
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self._create()
        self.early_exit = bool(early_exit)
        self.feature_store = None
        self.single_forward = False      # True: __call__ raises SingleForwardDone after one forward (stock diffusers pipelines)
        self.calls = 0                   # number of __call__ forwards so far (tests count one per pipe(...) call)
        self._range_check_sd = None      # state dict held for the first-forward activation range check (arm_range_check)
        self.range_check_log = None      # {"saturated": [(hook id, max |x|)], "mode_before": ..., "mode_after": ...} once the check has run
        self.config = types.SimpleNamespace(in_channels=cfg["in_channels"], guidance_embeds=bool(cfg["guidance_embeds"]),
                                            joint_attention_dim=cfg["joint_attention_dim"],
                                            pooled_projection_dim=cfg["pooled_projection_dim"])

    def _create(self):
        """(re)create the libgdf model for self.cfg["compute_dtype"]"""
        old = getattr(self, "handle", None)
        if old is not None:
            self.lib.gdf_model_destroy(old)
            self.handle = None
        self._desc = flux_desc(self.cfg)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_flux_model_create(C.byref(self._desc), C.byref(h)), "flux_model_create")
        self.handle = h
        self._plans = {}
        self.io_dtype = torch.float16 if self.cfg["compute_dtype"] in ("float16", "float16s", "auto") else torch.bfloat16   # inputs / `out` of libgdf
        self.dtype = self.io_dtype

    def _is_norm(self, name):
        return ".attn.norm_" in name

    def fp16_cast_report(self, sd):
        """'auto' guard: the worst relative Frobenius error any >= 2-D weight of `sd` loses when its values are cast to fp16 (bf16 checkpoints:
        exact for 6.1e-5 <= |w| <= 65504; smaller magnitudes lose bits, larger ones overflow) -> (worst error, its name)."""
        worst, wname = 0.0, None
        for name, shp in self.param_shapes().items():
            if len(shp) < 2 or name not in sd:
                continue
            t = sd[name]
            t = t.to(self.device, non_blocking=True).float()
            c = t.clamp(-65504.0, 65504.0).to(torch.float16).float()
            e = float((c - t).norm() / (t.norm() + 1e-30))
            if not (e <= worst):
                worst, wname = (e if e == e else float("inf")), name
            del t, c
        return worst, wname

    def load_state_dict(self, sd, strict=True):
        if self.cfg["compute_dtype"] == "auto":
            worst, wname = self.fp16_cast_report(sd)
            self.fp16_cast_error = worst
            if worst > self.FP16_CAST_TOL:
                import warnings
                warnings.warn(f"gdf flux 'auto': weight {wname} loses {worst:.1e} (> {self.FP16_CAST_TOL:.0e}) in the bf16 -> fp16 cast; loading the "
                              "checkpoint in 'bfloat16x2' mode (bf16 operand pairs) instead of 'float16s'", RuntimeWarning, stacklevel=2)
                self.cfg["compute_dtype"] = "bfloat16x2"
                self._create()
        return super().load_state_dict(sd, strict)

    # ---- activation range check of the fp16 modes on REAL checkpoints ----------------------------------------------
    def arm_range_check(self, sd):
        """Called by components/models.py for a checkpoint loaded from diffusers: if the model runs in an fp16 mode ('auto' / 'float16s' /
        'float16'), its FIRST forward is preceded by a one-sample forward that stores EVERY hook of EVERY block (q, k, v, attention output,
        modulated norm output, MLP hidden, block output: an image of each 16-bit tensor class of the MMDiT) and scans them for saturated
        (|x| = 65504: the kernels' 16-bit stores clamp) or non-finite values.  Any hit means an activation of THIS checkpoint leaves the fp16
        range somewhere the seeded synthetic weights never did: the weights in `sd` are re-loaded in 'bfloat16x2' (bf16's exponent range,
        hi + lo operand pairs) with one warning.  `sd` is released after the check.  GDF_FLUX_RANGE_CHECK=0 disables it."""
        if self.cfg["compute_dtype"] in ("auto", "float16s", "float16") and os.environ.get("GDF_FLUX_RANGE_CHECK", "1") not in ("", "0"):
            self._range_check_sd = sd
        return self

    def _run_range_check(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, grid):
        sd, self._range_check_sd = self._range_check_sd, None
        first = lambda v: v[:1] if (torch.is_tensor(v) and v.dim() > 0 and v.shape[0] > 1) else v
        ids = [h for h in self.hook_names() if not h.endswith("-map")]
        ee, self.early_exit = self.early_exit, False
        try:
            out, hooks = self.forward_raw(first(hidden_states), first(encoder_hidden_states), first(pooled_projections), first(timestep), img_ids,
                                          txt_ids, guidance=first(guidance) if guidance is not None else None, hook_ids=ids, grid=grid)
        finally:
            self.early_exit = ee
        FP16_MAX = 65504.0
        bad = []
        for k, v in list(hooks.items()) + [("output", out)]:
            m = float(v.float().abs().nan_to_num(nan=float("inf")).max())
            if not m < FP16_MAX:
                bad.append((k, m))
        del hooks, out
        self._plans.clear()
        before = self.cfg["compute_dtype"]
        if bad:
            import warnings
            warnings.warn(f"gdf flux: {len(bad)} 16-bit tensors of this checkpoint reach the end of the fp16 range in mode '{before}' (first: {bad[0][0]}, "
                          f"max |x| = {bad[0][1]:.3g}); re-loading the weights in 'bfloat16x2' (bf16 operand pairs, bf16's range)", RuntimeWarning, stacklevel=3)
            self.cfg["compute_dtype"] = "bfloat16x2"
            self._create()
            _NativeModel.load_state_dict(self, sd)
        self.range_check_log = {"saturated": bad, "mode_before": before, "mode_after": self.cfg["compute_dtype"], "tensors_scanned": len(ids) + 1}

    def _plan(self, batch, gh, gw, n_txt, hook_ids):
        key = (batch, gh, gw, n_txt, tuple(hook_ids), self.early_exit)
        p = self._plans.get(key)
        if p is None:
            ids = (C.c_char_p * max(1, len(hook_ids)))(*[s.encode() for s in hook_ids])
            opts = PlanOpts(1, int(self.early_exit))
            ph = C.c_void_p()
            _check(self.lib.gdf_flux_plan_create(self.handle, batch, gh, gw, n_txt, ids, len(hook_ids), C.byref(opts),
                                                 C.byref(ph)), "flux_plan_create")
            p = _Plan(self.lib, ph)
            if len(self._plans) >= 4:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def forward_raw(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
                    guidance=None, hook_ids=None, grid=None, profile=False):
        """Returns (output (B, S, in_channels) fp16, OrderedDict id -> hook tensor).  `grid` = (h, w) of the packed
        latent token grid; default: square (the reference's FeatureStore assumes it, feature_extractor.py:46-48)."""
        dev = self.device
        B, S, cin = hidden_states.shape
        if grid is None:
            g = int(round(S ** 0.5))
            if g * g != S:
                raise ValueError(f"{S} image tokens do not form a square grid; pass grid=(h, w)")
            grid = (g, g)
        x, enc, pooled = hidden_states, encoder_hidden_states, pooled_projections
        t = _timestep_on_device(timestep, B, dev)
        gd = None
        if self.cfg["guidance_embeds"]:
            if guidance is None:
                raise ValueError("guidance is required for a guidance-distilled transformer (guidance_embeds)")
            gd = torch.as_tensor(guidance, device=dev).float().reshape(-1)
            gd = gd.expand(B) if gd.numel() == 1 else gd
        img_ids = img_ids[0] if img_ids.dim() == 3 else img_ids           # transformer_flux.py:485-496
        txt_ids = txt_ids[0] if txt_ids.dim() == 3 else txt_ids
        T = enc.shape[1]
        if (cin != self.cfg["in_channels"] or tuple(enc.shape) != (B, T, self.cfg["joint_attention_dim"])
                or tuple(pooled.shape) != (B, self.cfg["pooled_projection_dim"]) or tuple(img_ids.shape) != (S, 3)
                or tuple(txt_ids.shape) != (T, 3)):
            raise ValueError("flux input shape mismatch")
        ids = list(hook_ids) if hook_ids is not None else self.requested_ids()
        plan = self._plan(B, grid[0], grid[1], T, ids)
        f16, f32 = self.io_dtype, torch.float32
        call = self._launch(plan, self.lib.gdf_flux_forward, self.lib.gdf_flux_plan_profile, "flux_forward", profile)
        out, feats, prof = plan.run(dev, [("x", x, f16), ("enc", enc, f16), ("pooled", pooled, f16), ("t", t, f32), ("gd", gd, f32),
                                          ("img_ids", img_ids, f32), ("txt_ids", txt_ids, f32)], (B, S, cin), call, profile=profile,
                                    out_dtype=f16)
        return (out, feats, prof) if profile else (out, feats)

    def __call__(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, img_ids=None,
                 txt_ids=None, guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None,
                 controlnet_single_block_samples=None, return_dict=True, grid=None, **kwargs):
        if controlnet_block_samples is not None or controlnet_single_block_samples is not None or joint_attention_kwargs:
            raise NotImplementedError("ControlNet residuals / IP-adapter kwargs are outside the native hot path")
        if self._range_check_sd is not None:
            self._run_range_check(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, grid)
        ids = self.requested_ids()
        out, hooks = self.forward_raw(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
                                      guidance=guidance, hook_ids=ids, grid=grid)
        self.calls += 1
        if self.feature_store is not None:
            for hid, t in hooks.items():
                self.feature_store.store(t, hid)
        if self.single_forward:
            # The reference's patched pipeline returns right after its FIRST transformer call
            # (feature/diffusers/pipelines/flux/pipeline_flux_img2img.py:804-841): one pipe(...) call = one denoiser forward at
            # sigmas[t_start].  A stock (un-patched) diffusers FluxImg2ImgPipeline would go on to scheduler.step, the remaining
            # steps and the VAE decode; FeatureExtractor.extract sets this flag and catches the exception instead.
            raise SingleForwardDone(out)
        if return_dict:
            return types.SimpleNamespace(sample=out)
        return (out,)


# --------------------------------------------------------------------------------------------- #
# VAE encoder + sampling + noise-add (include/gdf_vae.h): the step before the hot path
# --------------------------------------------------------------------------------------------- #
VAE_CONFIGS = {"sd": dict(in_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                          use_quant_conv=1),
               # FLUX.1 VAE: the SD block layout, 16 latent channels, no quant_conv (and a shift_factor, a run-time scalar of encode_packed)
               "flux": dict(in_channels=3, latent_channels=16, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                            use_quant_conv=0)}


class NativeVAEEncoder(_NativeModel):
    """AutoencoderKL encoder half + `latent_dist.sample()` + scaling + `scheduler.add_noise` + `scale_model_input` in
    libgdf.so — what `pipe.prepare_latents(...)` / `scheduler.scale_model_input` do at the reference's
    feature/diffusion_feature.py:371-380, :405-406.  Weights: `vae.state_dict()` entries "encoder.*" and "quant_conv.*"."""

    def __init__(self, cfg=None, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("NativeVAEEncoder needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg or VAE_CONFIGS["sd"])
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        d = self._desc = _vae_desc(self.cfg)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_vae_model_create(C.byref(d), C.byref(h)), "vae_model_create")
        self.handle = h
        self._plans = {}
        self.feature_store = None

    def _is_norm(self, name):
        return "norm" in name

    def load_vae_state_dict(self, sd):
        """Accepts a full `AutoencoderKL.state_dict()`: only the encoder / quant_conv entries are used."""
        return self.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")})

    def _plan(self, batch, h, w):
        key = (batch, h, w)
        p = self._plans.get(key)
        if p is None:
            ph = C.c_void_p()
            _check(self.lib.gdf_vae_plan_create(self.handle, batch, h, w, C.byref(ph)), "vae_plan_create")
            p = _Plan(self.lib, ph)
            # encode writes B latents, encode_multi up to MAX_TIMESTEPS * B: every output region of the plan holds the largest (16 MB for
            # 16 images at 1024^2), so both calls share the plan's buffer sets and the graphs recorded on them
            f = 1 << (len(self.cfg["block_out_channels"]) - 1)
            p.out_capacity = MAX_TIMESTEPS * batch * self.cfg["latent_channels"] * (h // f) * (w // f)
            if len(self._plans) >= 4:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def encode(self, image, eps=None, noise=None, scaling_factor=0.18215, noise_a=1.0, noise_b=0.0, input_scale=1.0,
               profile=False):
        """image (B,3,H,W) in [-1,1]; eps / noise (B,L,H/f,W/f) or None, f = 2^(levels-1) (8 for the SD VAEs).
        Returns (B,L,H/f,W/f) fp16: input_scale * (noise_a * scaling_factor * (mean + std * eps) + noise_b * noise)."""
        dev = self.device
        B, _, H, W = image.shape
        f = 1 << (len(self.cfg["block_out_channels"]) - 1)
        L = self.cfg["latent_channels"]
        for t in (eps, noise):
            if t is not None and tuple(t.shape) != (B, L, H // f, W // f):
                raise ValueError("eps / noise must have the latent shape (B, L, H/f, W/f)")
        plan = self._plan(B, H, W)
        lib = self.lib
        sc = (float(scaling_factor), float(noise_a), float(noise_b), float(input_scale))

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            args = (plan.handle, vp(staged[0]), vp(staged[1]), vp(staged[2])) + sc + (out_ptr, ws_ptr, stream_ptr)
            if not profile:
                _check(lib.gdf_vae_encode(*args), "vae_encode")
                return None
            n = lib.gdf_plan_num_ops(plan.handle)
            ms = (C.c_float * n)(); names = (C.c_char_p * n)(); fl = (C.c_double * n)()
            if lib.gdf_vae_plan_profile(*args, ms, names, fl, n) < 0:
                _check(1, "vae_plan_profile")
            return [(names[i].decode(), ms[i], fl[i], lib.gdf_plan_op_kernel(plan.handle, i).decode()) for i in range(n)]

        f16 = torch.float16
        out, _, prof = plan.run(dev, [("image", image, f16), ("eps", eps, f16), ("noise", noise, f16)], (B, L, H // f, W // f), call,
                                profile=profile)
        return (out, prof) if profile else out


    def encode_multi(self, image, eps=None, noise=None, scaling_factor=0.18215, noise_a=(1.0,), noise_b=(0.0,), input_scale=(1.0,)):
        """The same B images at K = len(noise_a) timesteps from ONE encoder pass (gdf_vae_encode_multi, on the plan and workspace encode uses).
        image (B,3,H,W); eps / noise (K*B,L,H/f,W/f) or None, TIMESTEP-MAJOR: row k*B + b is image b at timestep k.  noise_a, noise_b,
        input_scale: sequences of K floats.  Returns (K*B,L,H/f,W/f) fp16 whose rows k*B:(k+1)*B have the bits of
        encode(image, eps[k*B:(k+1)*B], noise[k*B:(k+1)*B], scaling_factor, noise_a[k], noise_b[k], input_scale[k])."""
        dev = self.device
        B, _, H, W = image.shape
        f = 1 << (len(self.cfg["block_out_channels"]) - 1)
        L = self.cfg["latent_channels"]
        K = len(noise_a)
        if not 1 <= K <= MAX_TIMESTEPS:
            raise ValueError(f"encode_multi takes 1..{MAX_TIMESTEPS} timesteps, got {K}")
        if len(noise_b) != K or len(input_scale) != K:
            raise ValueError("noise_a, noise_b and input_scale must have the same length")
        out_shape = (K * B, L, H // f, W // f)
        for t in (eps, noise):
            if t is not None and tuple(t.shape) != out_shape:
                raise ValueError("eps / noise must have the shape (K*B, L, H/f, W/f)")
        plan = self._plan(B, H, W)
        lib = self.lib
        arr = lambda v: (C.c_float * K)(*[float(x) for x in v])
        na, nb, sc = arr(noise_a), arr(noise_b), arr(input_scale)

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            _check(lib.gdf_vae_encode_multi(plan.handle, vp(staged[0]), vp(staged[1]), vp(staged[2]), float(scaling_factor), K, na, nb, sc,
                                            out_ptr, ws_ptr, stream_ptr), "vae_encode_multi")

        f16 = torch.float16
        # (staging buffers of their own names: eps / noise of encode have B rows, these K * B, and a plan serves both calls in turn)
        out, _, _ = plan.run(dev, [("image", image, f16), ("eps_multi", eps, f16), ("noise_multi", noise, f16)], out_shape, call)
        return out

    def encode_packed(self, image, eps=None, noise=None, scaling_factor=0.3611, shift_factor=0.1159, sigma=0.0, out_dtype=torch.float16):
        """The Flux latent preparation in one call (gdf_vae_encode_packed, on the plan and workspace encode uses): image (B,3,H,W) in [-1,1];
        eps / noise (B,L,H/f,W/f) or None.  Returns the 2x2-packed token rows (B, S, 4L), S = (H/2f)(W/2f), in `out_dtype` (fp16 or bf16):
        (1 - sigma) * scaling_factor * ((mean + std * eps) - shift_factor) + sigma * noise at [b, gy*(W/2f)+gx, c*4 + dy*2 + dx] for latent
        (b, c, 2gy+dy, 2gx+dx) — `_pack_latents(scheduler.scale_noise((z - shift) * scaling, t, noise))` of FluxImg2ImgPipeline."""
        dev = self.device
        B, _, H, W = image.shape
        f = 1 << (len(self.cfg["block_out_channels"]) - 1)
        L = self.cfg["latent_channels"]
        h, w = H // f, W // f
        if h % 2 or w % 2:
            raise ValueError("encode_packed needs an even latent grid (2x2 packing)")
        if out_dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("encode_packed writes fp16 or bf16 tokens")
        for t in (eps, noise):
            if t is not None and tuple(t.shape) != (B, L, h, w):
                raise ValueError("eps / noise must have the latent shape (B, L, H/f, W/f)")
        plan = self._plan(B, H, W)
        lib = self.lib
        sc = (float(scaling_factor), float(shift_factor), 1.0 - float(sigma), float(sigma), int(out_dtype == torch.bfloat16))

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            _check(lib.gdf_vae_encode_packed(plan.handle, vp(staged[0]), vp(staged[1]), vp(staged[2]), *sc, out_ptr, ws_ptr, stream_ptr),
                   "vae_encode_packed")

        f16 = torch.float16
        out, _, _ = plan.run(dev, [("image", image, f16), ("eps", eps, f16), ("noise", noise, f16)], (B, (h // 2) * (w // 2), 4 * L), call,
                             out_dtype=out_dtype)
        return out


def _vae_desc(cfg):
    d = VaeDesc()
    d.in_channels, d.latent_channels = cfg["in_channels"], cfg["latent_channels"]
    d.n_levels = len(cfg["block_out_channels"])
    for i, c in enumerate(cfg["block_out_channels"]):
        d.block_out_channels[i] = c
    d.layers_per_block = cfg["layers_per_block"]
    d.use_quant_conv = int(bool(cfg.get("use_quant_conv", 1)))
    return d


class NativeVAEDecoder(_NativeModel):
    """AutoencoderKL decoder half + the scheduler step in front of it, in libgdf.so — the optional `vae-out` feature of the reference
    (feature/diffusion_feature.py:60, :477-485: `latents = scheduler.step(noise_pred, t, latents)[0]`,
    `vae.decode(latents / scaling_factor)[0]`).  Weights: `vae.state_dict()` entries "decoder.*" and "post_quant_conv.*"."""

    def __init__(self, cfg=None, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("NativeVAEDecoder needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg or VAE_CONFIGS["sd"])
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self._desc = _vae_desc(self.cfg)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_vae_decoder_create(C.byref(self._desc), C.byref(h)), "vae_decoder_create")
        self.handle = h
        self._plans = {}
        self.feature_store = None

    def _is_norm(self, name):
        return "norm" in name

    def load_vae_state_dict(self, sd):
        """Accepts a full `AutoencoderKL.state_dict()`: only the decoder / post_quant_conv entries are used."""
        return self.load_state_dict({k: v for k, v in sd.items() if k.startswith("decoder.") or k.startswith("post_quant_conv.")})

    def _plan(self, batch, h, w):
        key = (batch, h, w)
        p = self._plans.get(key)
        if p is None:
            ph = C.c_void_p()
            _check(self.lib.gdf_vae_decode_plan_create(self.handle, batch, h, w, C.byref(ph)), "vae_decode_plan_create")
            p = _Plan(self.lib, ph)
            if len(self._plans) >= 4:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def decode(self, latents, noise_pred=None, c_sample=1.0, c_eps=0.0, scaling_factor=0.18215, profile=False):
        """latents / noise_pred (B,L,h,w); returns the image (B,3,8h,8w) fp16 (a channels-last view):
        decode((c_sample * latents + c_eps * noise_pred) / scaling_factor)."""
        dev = self.device
        B, L, h, w = latents.shape
        if noise_pred is not None and tuple(noise_pred.shape) != (B, L, h, w):
            raise ValueError("noise_pred must have the shape of the latents (B, L, h, w)")
        f = 1 << (len(self.cfg["block_out_channels"]) - 1)
        plan = self._plan(B, h, w)
        lib = self.lib
        sc = (float(c_sample), float(c_eps), 1.0 / float(scaling_factor))

        def call(staged, hook_ptrs, out_ptr, ws_ptr, stream_ptr):
            vp = lambda a: C.c_void_p(a.data_ptr() if a is not None else 0)
            args = (plan.handle, vp(staged[0]), vp(staged[1])) + sc + (out_ptr, ws_ptr, stream_ptr)
            if not profile:
                _check(lib.gdf_vae_decode(*args), "vae_decode")
                return None
            n = lib.gdf_plan_num_ops(plan.handle)
            ms = (C.c_float * n)(); names = (C.c_char_p * n)(); fl = (C.c_double * n)()
            if lib.gdf_vae_decode_plan_profile(*args, ms, names, fl, n) < 0:
                _check(1, "vae_decode_plan_profile")
            return [(names[i].decode(), ms[i], fl[i], lib.gdf_plan_op_kernel(plan.handle, i).decode()) for i in range(n)]

        f16 = torch.float16
        out, _, prof = plan.run(dev, [("latents", latents, f16), ("noise_pred", noise_pred, f16)], (B, h * f, w * f, self.cfg["in_channels"]),
                                call, profile=profile)
        img = out.permute(0, 3, 1, 2)                       # logical (B,3,H,W), stored channels-last like the hooks
        return (img, prof) if profile else img


# --------------------------------------------------------------------------------------------- #
# PixArt DiT (include/gdf_pixart.h): Transformer2DModel `config.json` of PixArt-alpha/PixArt-Sigma-XL-2-1024-MS
# (reference components/models.py:72-111)
# --------------------------------------------------------------------------------------------- #
PIXART_CONFIGS = {
    "pixart-sigma": dict(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=28,
                         patch_size=2, sample_size=128, caption_channels=4096, interpolation_scale=2),
    "pixart-sigma-512": dict(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=28,
                             patch_size=2, sample_size=64, caption_channels=4096, interpolation_scale=1),
    # PixArt-alpha/PixArt-XL-2-512x512 (reference models.py:103-115): the same 28-block DiT; at sample_size 64 the checkpoint has no
    # resolution / aspect-ratio micro-conditioning (`use_additional_conditions` is only set at sample_size 128) and the reference
    # calls it with added_cond_kwargs = {'resolution': None, 'aspect_ratio': None} (diffusion_feature.py:466-474)
    "pixart-alpha": dict(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=28,
                         patch_size=2, sample_size=64, caption_channels=4096, interpolation_scale=1),
}


class NativePixArtTransformer(_NativeModel):
    """Transformer2DModel (PixArt, ada_norm_single) replacement running entirely in libgdf.so.

    Call signature mirrors the reference's use at feature/diffusion_feature.py:466-474:
        transformer(latent_model_input, encoder_hidden_states=prompt_embeds, encoder_attention_mask=prompt_attention_mask,
                    timestep=t, return_dict=False, added_cond_kwargs={'resolution': None, 'aspect_ratio': None})[0]
    Hook ids `vit-block{i}-{self-q,self-k,self-v,cross-q,ffn-inner,out}` (components/feature_extractor.py:250-286)."""

    def __init__(self, cfg, device="cuda", early_exit=False):
        if not torch.cuda.is_available():
            raise RuntimeError("NativePixArtTransformer needs an MI355X (HIP device); there is no CPU fallback")
        self.lib = load_library()
        self.cfg = dict(cfg)
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        d = PixartDesc()
        for k, _ in PixartDesc._fields_:
            setattr(d, k, int(cfg[k]))
        self._desc = d
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _create(lambda: self.lib.gdf_pixart_model_create(C.byref(d), C.byref(h)), "pixart_model_create")
        self.handle = h
        self.early_exit = bool(early_exit)
        self.feature_store = None
        self._plans = {}
        self.dtype = torch.float16
        self.io_dtype = torch.float16
        self.extra_hook_ids = []         # '-map' hooks FeatureExtractor needs internally (aggregated `attention=` feature)
        self.last_extra = {}
        self.config = types.SimpleNamespace(in_channels=cfg["in_channels"], sample_size=cfg["sample_size"],
                                            out_channels=cfg["out_channels"])

    def init_synthetic(self, seed=0, **kw):
        """Linear weights ~ N(0, 1/fan_in), biases 0.05 N, scale_shift_table ~ N(0, 1/C) (transformer_2d.py:304)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        stream = torch.cuda.current_stream(self.device)
        c = self.cfg["num_attention_heads"] * self.cfg["attention_head_dim"]
        with torch.cuda.device(self.device):
            for name, shp in self.param_shapes().items():
                t = torch.randn(shp, generator=g, device=self.device, dtype=torch.float32)
                if name.endswith("scale_shift_table"):
                    t.mul_(c ** -0.5)
                elif name.endswith(".weight"):
                    fan = 1
                    for s_ in shp[1:]:
                        fan *= s_
                    t.mul_(fan ** -0.5)
                else:
                    t.mul_(0.05)
                t = t.half()
                _check(self.lib.gdf_model_set_param(self.handle, name.encode(), C.c_void_p(t.data_ptr()), GDF_F16,
                                                    C.c_void_p(stream.cuda_stream)), f"set_param({name})")
                stream.synchronize()
        return self

    def _plan(self, batch, h, w, n_txt, hook_ids):
        key = (batch, h, w, n_txt, tuple(hook_ids), self.early_exit)
        p = self._plans.get(key)
        if p is None:
            ids = (C.c_char_p * max(1, len(hook_ids)))(*[s.encode() for s in hook_ids])
            opts = PlanOpts(1, int(self.early_exit))
            ph = C.c_void_p()
            _check(self.lib.gdf_pixart_plan_create(self.handle, batch, h, w, n_txt, ids, len(hook_ids), C.byref(opts),
                                                   C.byref(ph)), "pixart_plan_create")
            p = _Plan(self.lib, ph)
            if len(self._plans) >= 4:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = p
        return p

    def forward_raw(self, hidden_states, encoder_hidden_states, timestep, encoder_attention_mask=None, hook_ids=None,
                    profile=False):
        """Returns (output (B, out_channels, H, W) fp16, OrderedDict id -> hook tensor)."""
        dev = self.device
        B, cin, H, W = hidden_states.shape
        x, enc = hidden_states, encoder_hidden_states
        t = _timestep_on_device(timestep, B, dev)
        T = enc.shape[1]
        if cin != self.cfg["in_channels"] or tuple(enc.shape) != (B, T, self.cfg["caption_channels"]):
            raise ValueError("pixart input shape mismatch")
        lens = None
        if encoder_attention_mask is not None:
            m = encoder_attention_mask.to(dev).reshape(B, T) > 0.5
            lens = m.sum(1).to(torch.int32)
            if not torch.equal(m, torch.arange(T, device=dev)[None] < lens[:, None]):
                raise NotImplementedError("encoder_attention_mask must keep a leading prefix of the caption tokens")
        ids = list(hook_ids) if hook_ids is not None else self.requested_ids()
        plan = self._plan(B, H, W, T, ids)
        f16 = self.io_dtype
        call = self._launch(plan, self.lib.gdf_pixart_forward, self.lib.gdf_pixart_plan_profile, "pixart_forward", profile)
        out, feats, prof = plan.run(dev, [("x", x, f16), ("t", t, torch.float32), ("enc", enc, f16), ("lens", lens, torch.int32)],
                                    (B, self.cfg["out_channels"], H, W), call, profile=profile)
        return (out, feats, prof) if profile else (out, feats)

    def __call__(self, hidden_states, encoder_hidden_states=None, timestep=None, added_cond_kwargs=None,
                 encoder_attention_mask=None, return_dict=True, **kwargs):
        akw = added_cond_kwargs or {}
        if akw.get("resolution") is not None or akw.get("aspect_ratio") is not None:
            raise NotImplementedError("PixArt-alpha micro-conditioning (use_additional_conditions) is not native")
        ids = self.requested_ids()
        have = set(ids)
        ids = ids + [i for i in self.extra_hook_ids if i not in have]
        out, hooks = self.forward_raw(hidden_states, encoder_hidden_states, timestep, encoder_attention_mask, hook_ids=ids)
        self.last_extra = {k: v for k, v in hooks.items() if k in set(self.extra_hook_ids)}
        if self.feature_store is not None:
            for hid, tens in hooks.items():
                if hid in have:
                    self.feature_store.store(tens, hid)
        if return_dict:
            return types.SimpleNamespace(sample=out)
        return (out,)
