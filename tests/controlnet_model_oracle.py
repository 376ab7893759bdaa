"""CPU oracle of the ControlNet model (test infrastructure).

controlnet_forward restates diffusers' ControlNetModel.forward (0.32.2) for conditioning_scale = 1, guess_mode = False, no class
embedding: the UNet's time / add embedding, `conv_in(sample) + controlnet_cond_embedding(cond)`, the UNet's down blocks collecting the skip
list, the UNet's mid block, and one 1x1 conv per skip and for the mid block's output.  The class is not vendored in the reference tree
(/root/reference/feature/components/controlnet.py imports it from an installed diffusers), so this wiring is restated from the published
source and is NOT pinned by a golden vector of the reference's own run — the same status as the `unet_2d_blocks` containers.
The blocks it is built from — oracle.unet_ref's time_embed, resnet_block, transformer_2d and downsample — are pinned to the reference at 2e-5
by tests/test_oracle_golden.py, and unet_forward_res (tests/controlnet_oracle.py), which consumes its outputs, by
tests/test_controlnet_cpu.py.

Everything goes through torch.nn.functional at call time, so oracle.operand_floor.fp16_operands() applies."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import unet_ref as R

COND_CHANNELS = (16, 32, 96, 256)


def cond_embedding(P, cond, cond_channels=COND_CHANNELS):
    """controlnet_cond_embedding: conv_in, SiLU; blocks.0..5 (stride 1, 2, 1, 2, 1, 2), each + SiLU; conv_out"""
    p = "controlnet_cond_embedding."
    h = F.silu(F.conv2d(cond.float(), P[p + "conv_in.weight"], P[p + "conv_in.bias"], padding=1))
    for i in range(2 * (len(cond_channels) - 1)):
        h = F.silu(F.conv2d(h, P[p + f"blocks.{i}.weight"], P[p + f"blocks.{i}.bias"], padding=1, stride=1 + i % 2))
    return F.conv2d(h, P[p + "conv_out.weight"], P[p + "conv_out.bias"], padding=1)


def controlnet_forward(P, arch, sample, timestep, ctx, text_embeds=None, time_ids=None, cond=None, cond_channels=COND_CHANNELS):
    """-> (list of down residuals in diffusers' skip order, mid residual), fp32 (B, C, H, W)"""
    store = R.Store({"-": True})                 # a ControlNet registers no hooks: nothing is stored
    boc = arch["block_out_channels"]
    L, nl = len(boc), arch["layers_per_block"]
    sample, ctx = sample.float(), ctx.float()
    if timestep.dim() == 0:
        timestep = timestep[None]
    timestep = timestep.expand(sample.shape[0])
    emb = R.time_embed(P, arch, timestep, text_embeds, time_ids, None)
    h = F.conv2d(sample, P["conv_in.weight"], P["conv_in.bias"], padding=1) + cond_embedding(P, cond, cond_channels)
    skips = [h]
    for lv in range(L):
        for r in range(nl):
            h = R.resnet_block(P, f"down_blocks.{lv}.resnets.{r}", h, emb, store, f"down-level{lv}-repeat{r}-res")
            if arch["down_attn"][lv]:
                h = R.transformer_2d(P, f"down_blocks.{lv}.attentions.{r}", h, ctx, arch["heads"][lv], arch["transformer_layers"][lv],
                                     arch["linear_proj"], store, f"down-level{lv}-repeat{r}-vit", False)
            skips.append(h)
        if lv != L - 1:
            h = R.downsample(P, f"down_blocks.{lv}.downsamplers.0", h, store, f"down-level{lv}-downsampler")
            skips.append(h)
    h = R.resnet_block(P, "mid_block.resnets.0", h, emb, store, "mid-repeat0-res")
    h = R.transformer_2d(P, "mid_block.attentions.0", h, ctx, arch["heads"][-1], arch["transformer_layers"][-1], arch["linear_proj"], store,
                         "mid-vit", False)
    h = R.resnet_block(P, "mid_block.resnets.1", h, emb, store, "mid-repeat1-res")
    down = [F.conv2d(s, P[f"controlnet_down_blocks.{k}.weight"], P[f"controlnet_down_blocks.{k}.bias"]) for k, s in enumerate(skips)]
    mid = F.conv2d(h, P["controlnet_mid_block.weight"], P["controlnet_mid_block.bias"])
    return down, mid


def controlnet_param_shapes(arch, cond_channels=COND_CHANNELS, conditioning_channels=3):
    """diffusers' ControlNetModel state-dict names and shapes: the UNet's encoder names, the embedding convs and the 1x1 convs"""
    boc = arch["block_out_channels"]
    S = OrderedDict((k, v) for k, v in R.param_shapes(arch).items()
                    if k.startswith(("conv_in.", "time_embedding.", "add_embedding.", "down_blocks.", "mid_block.")))
    p = "controlnet_cond_embedding."
    cc = tuple(cond_channels)

    def conv(n, co, ci, k):
        S[n + ".weight"] = (co, ci, k, k)
        S[n + ".bias"] = (co,)
    conv(p + "conv_in", cc[0], conditioning_channels, 3)
    for i in range(len(cc) - 1):
        conv(p + f"blocks.{2 * i}", cc[i], cc[i], 3)
        conv(p + f"blocks.{2 * i + 1}", cc[i + 1], cc[i], 3)
    conv(p + "conv_out", boc[0], cc[-1], 3)
    widths = [boc[0]]
    for lv in range(len(boc)):
        widths += [boc[lv]] * arch["layers_per_block"]
        if lv != len(boc) - 1:
            widths.append(boc[lv])
    for k, c in enumerate(widths):
        conv(f"controlnet_down_blocks.{k}", c, c, 1)
    conv("controlnet_mid_block", boc[-1], boc[-1], 1)
    return S


def synth_controlnet_params(arch, seed=0, cond_channels=COND_CHANNELS, conditioning_channels=3):
    """Seeded synthetic ControlNet weights: oracle.unet_ref.synth_params restricted to the encoder names, plus the embedding convs and the
    1x1 convs, ALL with non-zero N(0, 1 / fan_in) weights and 0.05 N biases (a checkpoint's zero-initialised convs would make every parity
    test vacuous); fp16-representable."""
    U = R.synth_params(arch, seed=seed)
    g = torch.Generator().manual_seed(seed + 4099)
    P = OrderedDict()
    for name, shape in controlnet_param_shapes(arch, cond_channels, conditioning_channels).items():
        if name in U:
            P[name] = U[name]
        elif name.endswith(".weight"):
            P[name] = (torch.randn(shape, generator=g) / math.sqrt(shape[1] * shape[2] * shape[3])).half().float()
        else:
            P[name] = (0.05 * torch.randn(shape, generator=g)).half().float()
    return P


def synth_cond(batch, lat_h, lat_w=None, seed=3, channels=3):
    """a control image as VaeImageProcessor(do_normalize=False) hands it over: 8-bit values / 255 in [0, 1], rounded to fp16"""
    lat_w = lat_h if lat_w is None else lat_w
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (batch, channels, 8 * lat_h, 8 * lat_w), generator=g).float() / 255.0).half().float()
