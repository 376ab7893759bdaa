"""ctypes binding of include/gdf_ops.h for the kernel-level GPU tests."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
from components import native  # noqa: E402

vp, ci, fp = C.c_void_p, C.c_int, C.c_float


class AttnArgs(C.Structure):
    """gdf_attn_args of include/gdf_ops.h (same field order)"""
    _fields_ = [("q", vp), ("ldq", ci), ("k", vp), ("ldk", ci), ("v", vp), ("ldv", ci), ("o", vp), ("ldo", ci),
                ("B", ci), ("heads", ci), ("Sq", ci), ("Sk", ci), ("D", ci), ("kv_bstride", ci), ("scale", fp),
                ("map", vp), ("map2", vp), ("kv_len", vp), ("seg_T", ci), ("bf16", ci), ("o_lo", ci), ("o_pair_bf16", ci),
                ("q_lo", ci), ("kv_lo", ci), ("o_scale", fp)]


class GemmArgs(C.Structure):
    """gdf_gemm_args of include/gdf_ops.h (same field order)"""
    _fields_ = [("A", vp), ("lda", ci), ("W", vp), ("mode", ci), ("M", ci), ("N", ci), ("K", ci),
                ("B", ci), ("H", ci), ("Wd", ci), ("Cin", ci), ("stride", ci), ("ups", ci), ("pad0", ci),
                ("bias", vp), ("rowvec", vp), ("rows_per_sample", ci), ("ldrv", ci),
                ("res32", vp), ("res16", vp), ("ldres", ci), ("out16", vp), ("ldo16", ci), ("out32", vp), ("ldo32", ci),
                ("aux16", vp), ("ldaux", ci), ("geglu", ci), ("bn", ci), ("variant", ci), ("no_superblock", ci),
                ("splitk", ci), ("splitk_ws", vp), ("batch", ci), ("w_bstride", C.c_long), ("o_bstride", C.c_long),
                ("dit", ci), ("act", ci), ("rv_mul", ci), ("rv_seg_rows", ci), ("rv_rps2", ci), ("rv_tok", ci),
                ("qkn_nq", ci), ("qkn_wq", vp), ("qkn_wk", vp), ("qkn_eps", fp), ("rope_cos", vp), ("rope_sin", vp),
                ("qkn_pos0", ci), ("qkn_rps", ci), ("qkn_seg_rows", ci), ("qkn_pos1", ci), ("qkn_rps2", ci),
                ("bf16", ci), ("out_f16", ci), ("acc_scale", fp), ("out16_scale", fp), ("a_lo", ci), ("o16_lo", ci),
                ("cus", ci), ("mx", ci)]


OPS = {
    "gdf_op_gemm": (ci, [vp, ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp]),
    "gdf_op_gemm_ex": (ci, [C.POINTER(GemmArgs), vp]),
    "gdf_op_gemm_kernel": (C.c_char_p, [C.POINTER(GemmArgs)]),
    "gdf_op_conv3x3": (ci, [vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp, ci, vp]),
    "gdf_op_conv_in": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp]),
    "gdf_op_gemm_split": (ci, [vp, ci, ci, vp, vp, vp, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, vp]),
    "gdf_op_conv3x3_split": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, vp, vp, ci, ci, vp, vp]),
    "gdf_op_layernorm_split": (ci, [vp, ci, ci, ci, fp, vp, vp, vp, ci, ci, vp]),
    "gdf_op_groupnorm_split": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, fp, vp, vp, ci, vp, ci, ci, vp, vp]),
    "gdf_op_attention_split": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_attention_pair": (ci, [vp, ci, vp, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    "gdf_op_attention_ex": (ci, [C.POINTER(AttnArgs), vp]),
    "gdf_op_attention_kernel": (C.c_char_p, [C.POINTER(AttnArgs)]),
    "gdf_op_attention": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_groupnorm_scratch_bytes": (C.c_size_t, [ci, ci, ci]),
    "gdf_op_groupnorm": (ci, [vp, vp, ci, ci, ci, ci, ci, fp, vp, vp, ci, vp, vp, vp]),
    "gdf_op_gn_path": (ci, [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
    "gdf_op_gn_stats": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, fp, vp, vp, vp, vp, vp]),
    "gdf_op_gn_apply": (ci, [vp, ci, vp, ci, ci, ci, ci, vp, ci, vp, ci, ci, vp]),
    "gdf_op_gn_finalize": (ci, [vp, ci, ci, ci, ci, ci, fp, vp, vp, vp, vp, vp]),
    "gdf_op_gn_fold_floats": (C.c_size_t, [ci, ci, ci]),
    "gdf_op_conv3x3_gn": (ci, [vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp, ci, fp, vp, vp]),
    "gdf_op_conv_in_gn": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, fp, vp, vp]),
    "gdf_op_conv3x3_gn_info": (C.c_char_p, [ci, ci, ci, ci, ci, ci, ci, ci, C.POINTER(ci)]),
    "gdf_op_layernorm": (ci, [vp, vp, ci, ci, ci, fp, vp, vp, vp, vp]),
    "gdf_op_copy2d": (ci, [vp, vp, ci, vp, ci, ci, ci, vp]),
    "gdf_op_copy2d_ex": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, fp, vp]),
    "gdf_op_sinusoid": (ci, [vp, ci, ci, ci, vp, ci, ci, ci, fp, vp]),
    "gdf_op_widen": (ci, [vp, ci, ci, ci, vp, ci, ci, vp]),
    "gdf_op_silu_vec": (ci, [vp, vp, C.c_long, vp]),
    "gdf_op_add_table": (ci, [vp, vp, ci, ci, ci, C.c_long, vp, C.c_long, vp]),
    "gdf_op_pack_latents": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "gdf_op_patchify": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_unpatchify": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_vae_finish": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, fp, fp, fp, fp, vp, vp]),
    "gdf_op_vae_dec_prepare": (ci, [vp, vp, ci, ci, ci, fp, fp, fp, vp, vp, vp, vp]),
    "gdf_op_relayout_rows_padk": (ci, [vp, ci, vp, ci, ci, ci, vp]),
    "gdf_op_relayout_conv": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]),
    "gdf_op_relayout_rows": (ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp]),
    "gdf_op_relayout_vec": (ci, [vp, ci, vp, ci, ci, ci, vp]),
    "gdf_op_relayout_conv3": (ci, [vp, vp, ci, ci, vp]),
    "gdf_op_relayout_geglu": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "gdf_op_sincos_pos_embed": (ci, [vp, ci, ci, ci, ci, fp, vp]),
    "gdf_op_softmax_rows": (ci, [vp, ci, ci, ci, fp, vp]),
    "gdf_op_small_linear": (ci, [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp, ci, vp]),
    "gdf_op_small_linear_ex": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp, ci, vp]),
    "gdf_op_resize_concat": (ci, [vp, ci, C.c_long, C.c_long, C.c_long, C.c_long, ci, ci, ci, ci, vp, ci, ci, ci, vp]),
    "gdf_op_avg_pool": (ci, [vp, C.c_long, C.c_long, C.c_long, ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_maps_mean": (ci, [C.POINTER(vp), ci, ci, ci, ci, ci, vp, vp]),
    "gdf_op_set_e16": (ci, [ci]),
    "gdf_op_gemm_dit": (ci, [vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp]),
    "gdf_op_quant_rows_fp8": (ci, [vp, ci, ci, ci, ci, vp, ci, vp, vp]),
    "gdf_op_gemm_mx": (ci, [vp, ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, vp]),
    "gdf_op_layernorm_mod": (ci, [vp, ci, ci, ci, fp, vp, vp, ci, ci, ci, ci, vp, vp]),
    "gdf_op_layernorm_mod_ex": (ci, [vp, vp, ci, ci, ci, fp, vp, vp, ci, ci, ci, ci, vp, ci, ci, ci, vp, ci, vp, vp]),
    "gdf_op_layernorm_mod_path": (ci, [ci]),
    "gdf_op_qk_norm_rope": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, fp, vp, vp, ci, ci, vp]),
    "gdf_op_rope_table": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, vp]),
    "gdf_op_attention_joint": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]),
}


def lib():
    L = native.load_library()
    for n, (r, a) in OPS.items():
        f = getattr(L, n)
        f.restype, f.argtypes = r, a
    return L


def P(t):
    return vp(t.data_ptr()) if t is not None else vp(0)


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def ok(rc, L):
    assert rc == 0, L.gdf_last_error().decode()


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))
