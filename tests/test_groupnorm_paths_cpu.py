"""The GroupNorm coverage contract, checked without a GPU: every kernel form that a GroupNorm site of SD1.5 / 2.1 / SDXL or of the VAE
reaches at the benchmark sizes (batches 1, 2 and 16) has a kernel-level case in tests/test_gpu_groupnorm.py, and the emulated
summation order of every case stays within a third of the bounds that file asserts on the GPU.  Host arithmetic only
(gdf_op_gn_path, gdf_op_conv3x3_gn_info, gdf_op_gn_fold_floats).

A form is one of
  ("fused", channels per group)                          gn_fused_kernel
  ("partial", row groups, column loop, unrolled loop)    gn_partial_kernel
  ("finalize", channels per group)                       gn_finalize_kernel
  ("epilogue", kernel symbol)                            the conv whose epilogue leaves the per-slab sums
  ("fold", (threads per slab row, row groups) | None)    gn_fold_kernel in front of the finalize, or the unfolded gather
A site whose input may or may not carry sums from its producer (that depends on buffer ownership in the plan) counts for both ways."""
import pytest

from ops_binding import lib
from test_gpu_groupnorm import (CASES, CONV_CASES, FOLD_CASES, K128, K160, K256, K826, K932, KIN, NORM_CASES, case_forms, conv_info, fold_shape,
                                gn_path, partial_form, run_conv_case, run_norm_case)

from components import native

BATCHES = (1, 2, 16)


def site_forms(L, B, H, W, C, producer=None):
    """forms of one GroupNorm(32) over (B, H, W, C); producer = (Cin, stride, ups) of the 3x3 conv that wrote the tensor, or None"""
    HW, cpg = H * W, C // 32
    sc, slab, _ = gn_path(L, B, HW, C, 32)
    if sc:
        return {("fused", cpg)}
    forms = {("partial",) + partial_form(C, slab), ("finalize", cpg)}
    if producer:
        cin, stride, ups = producer
        name, rows = conv_info(L, B, H * stride // (2 if ups else 1), W * stride // (2 if ups else 1), cin, C, stride, ups, 0)
        if name and HW % rows == 0:
            nslab = HW // rows
            forms |= {("epilogue", name), ("fold", fold_shape(nslab, C) if L.gdf_op_gn_fold_floats(B, nslab, C) else None)}
    return forms


def unet_forms(L, cfg, side, B):
    boc, lpb = cfg["block_out_channels"], cfg["layers_per_block"]
    forms, skips = set(), [boc[0]]
    c, h = boc[0], side
    for i, co in enumerate(boc):                                             # down path: norm1 / norm2 of every resnet, the transformer's norm
        for _ in range(lpb):
            forms |= site_forms(L, B, h, h, c, (c, 1, 0)) | site_forms(L, B, h, h, co, (c, 1, 0))
            if cfg["has_attn"][i]:
                forms |= site_forms(L, B, h, h, co, (co, 1, 0))
            c = co
            skips.append(c)
        if i != len(boc) - 1:
            skips.append(c)
            h //= 2
    for _ in range(2):                                                       # mid block
        forms |= site_forms(L, B, h, h, c, (c, 1, 0))
    for i in reversed(range(len(boc))):                                      # up path: norm1 sees the skip concat
        co = boc[i]
        for _ in range(lpb + 1):
            cin = c + skips.pop()
            forms |= site_forms(L, B, h, h, cin) | site_forms(L, B, h, h, co, (cin, 1, 0))
            if cfg["has_attn"][i]:
                forms |= site_forms(L, B, h, h, co, (co, 1, 0))
            c = co
        if i != 0:
            h *= 2
    return forms | site_forms(L, B, h, h, c, (c, 1, 0))                      # conv_norm_out


def vae_forms(L, cfg, image, B):
    boc, lpb = cfg["block_out_channels"], cfg["layers_per_block"]
    forms = set()
    c, h = boc[0], image
    forms |= site_forms(L, B, h, h, c, (cfg["in_channels"], 1, 0))           # encoder: conv_in feeds the first norm1
    for i, co in enumerate(boc):
        for _ in range(lpb):
            forms |= site_forms(L, B, h, h, c, (c, 1, 0)) | site_forms(L, B, h, h, co, (c, 1, 0))
            c = co
        if i != len(boc) - 1:
            h //= 2
            forms |= site_forms(L, B, h, h, c, (c, 2, 0))                    # after the stride-2 downsampler
    forms |= site_forms(L, B, h, h, c, (c, 1, 0))                            # mid resnets, mid attention norm, conv_norm_out
    for i in reversed(range(len(boc))):                                      # decoder
        co = boc[i]
        for _ in range(lpb + 1):
            forms |= site_forms(L, B, h, h, c, (c, 1, 0)) | site_forms(L, B, h, h, co, (c, 1, 0))
            c = co
        if i != 0:
            h *= 2
            forms |= site_forms(L, B, h, h, c, (c, 1, 1))                    # after the upsampler's conv
    return forms | site_forms(L, B, h, h, c, (c, 1, 0))


def production_forms(L):
    forms = set()
    for key, side in (("1-5", 64), ("2-1", 64), ("xl", 128)):
        for B in BATCHES:
            forms |= unet_forms(L, native.ARCH_CONFIGS[key], side, B)
    for image in (512, 1024):
        for B in BATCHES:
            forms |= vae_forms(L, native.VAE_CONFIGS["sd"], image, B)
    return forms


def forms_with_a_case(L):
    forms = set()
    for c in CASES:
        forms |= case_forms(c, L)
    for nslab, C in FOLD_CASES:
        forms |= {("fold", fold_shape(nslab, C)), ("finalize", C // 32)}
    return forms


def test_case_ids_are_unique_and_conv_cases_name_their_kernel():
    L = lib()
    assert len({c["id"] for c in CASES}) == len(CASES)
    for c in CONV_CASES:
        name, slab = conv_info(L, c["B"], c["H"], c["W"], 4 if c.get("conv_in") else 64, c["C"], c.get("stride", 1), c.get("ups", 0), c["variant"])
        assert (name, slab) == (c["kernel"], 128 if c["kernel"] == K932 else 64), (c["id"], name, slab)
    assert {c["kernel"] for c in CONV_CASES} == {K128, K160, K256, K826, K932, KIN}      # all six instantiations


def test_every_form_the_models_reach_has_a_case():
    L = lib()
    tested, production = forms_with_a_case(L), production_forms(L)
    report = "\ntested:\n  %s\nproduction:\n  %s\n" % tuple("\n  ".join(sorted(map(repr, s))) for s in (tested, production))
    assert production <= tested, "forms without a kernel test: %s%s" % (sorted(map(repr, production - tested)), report)


def test_documented_paths():
    """spot checks of the choices the table of cases relies on"""
    L = lib()
    assert gn_path(L, 1, 4096, 320, 32) == (0, 16, 256)                      # above 32 x 32 pixels: the statistics pass, slab 16
    assert gn_path(L, 2, 65536, 64, 32)[:2] == (0, 64)
    assert gn_path(L, 2, 1024, 384, 32)[0] == 96                             # 12 channels per group: lcm(12, 8) = 24 -> 96
    assert gn_path(L, 16, 1024, 1280, 32)[0] == 80
    assert conv_info(L, 16, 128, 128, 320, 320, 1, 0, 0) == (K932, 128)      # SDXL level 0: the 256x320 tile, 128-row slabs
    assert conv_info(L, 1, 1024, 1024, 128, 128, 1, 0, 0) == (K256, 64)      # VAE level 0
    assert conv_info(L, 1, 256, 256, 512, 512, 1, 0, 0) == (K826, 64)
    assert conv_info(L, 1, 6, 6, 64, 64, 1, 0, 0) == (None, 0)               # M % 64 != 0
    assert fold_shape(300, 512) == (256, 1) and fold_shape(300, 256) == (128, 2) and fold_shape(300, 320) is None
    assert L.gdf_op_gn_fold_floats(2, 256, 64) == 0 and L.gdf_op_gn_fold_floats(2, 257, 64) == 2 * 128 * 64 * 2


@pytest.mark.parametrize("c", NORM_CASES, ids=[c["id"] for c in NORM_CASES])
def test_emulated_summation_leaves_the_bounds_their_headroom(c):
    run_norm_case(c, gpu=False)


@pytest.mark.parametrize("c", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_emulated_epilogue_sums_leave_the_bounds_their_headroom(c):
    run_conv_case(c, gpu=False)
