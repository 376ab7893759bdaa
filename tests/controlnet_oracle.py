"""CPU oracle of the ControlNet-conditioned UNet forward (test infrastructure).

Built from oracle.unet_ref's own block functions (time_embed, resnet_block, transformer_2d, downsample, upsample) and F.conv2d /
F.group_norm looked up through torch.nn.functional at call time, so oracle.operand_floor.fp16_operands() applies to it exactly as to
oracle.unet_ref.unet_forward.

unet_forward_res restates UNet2DConditionModel.forward with `down_block_additional_residuals` / `mid_block_additional_residual`
(reference feature/diffusers/models/unet/unet_2d_condition.py:1194, 1236-1245, 1269-1270): every entry of the skip list gets its residual
added as a NEW tensor after the down loop (the running sample that enters the mid block is unchanged), and the mid block's output gets the
mid residual.  tests/golden/unet_tiny_residuals_*.npz (gen_golden_controlnet.py) pins it against the reference's own forward."""
import torch
import torch.nn.functional as F

from oracle import unet_ref as R


def residual_shapes(arch, batch, lat_h, lat_w=None):
    """[(B, C, H, W)] of down_block_additional_residuals in diffusers' order — the conv_in output, then per level every resnet
    (+ transformer) output and, on all but the last level, the downsampler output — and the shape of the mid residual."""
    lat_w = lat_h if lat_w is None else lat_w
    boc = arch["block_out_channels"]
    L, nl = len(boc), arch["layers_per_block"]
    h, w = lat_h, lat_w
    down = [(batch, boc[0], h, w)]
    for lv in range(L):
        down += [(batch, boc[lv], h, w)] * nl
        if lv != L - 1:
            h, w = h // 2, w // 2
            down.append((batch, boc[lv], h, w))
    return down, (batch, boc[-1], h, w)


def synth_residuals(arch, batch, lat_h, lat_w=None, seed=7, scale=0.5):
    """Seeded residuals, exactly representable in fp16 (the dtype the native path takes them in) -> (list of down residuals, mid residual)"""
    g = torch.Generator().manual_seed(seed)
    down, mid = residual_shapes(arch, batch, lat_h, lat_w)
    mk = lambda s: (scale * torch.randn(s, generator=g)).half().float()
    return [mk(s) for s in down], mk(mid)


def unet_forward_res(P, arch, sample, timestep, ctx, text_embeds=None, time_ids=None, down_res=None, mid_res=None, store=None,
                     want_map=None, act_dtype=None):
    """oracle.unet_ref.unet_forward with the ControlNet residuals; down_res = mid_res = None is that function."""
    store = store or R.Store()
    if want_map is None:
        want_map = store.accept_all or any("map" in k and v for k, v in store.to_store.items())
    boc = arch["block_out_channels"]
    L, nl = len(boc), arch["layers_per_block"]
    sample, ctx = sample.float(), ctx.float()
    if timestep.dim() == 0:
        timestep = timestep[None]
    timestep = timestep.expand(sample.shape[0])
    emb = R.time_embed(P, arch, timestep, text_embeds, time_ids, act_dtype)

    store.gather("unet", sample, "in")
    h = F.conv2d(sample, P["conv_in.weight"], P["conv_in.bias"], padding=1)
    store.gather("unet", h, "after-conv-in")
    skips = [h]
    for lv in range(L):
        for r in range(nl):
            h = R.resnet_block(P, f"down_blocks.{lv}.resnets.{r}", h, emb, store, f"down-level{lv}-repeat{r}-res")
            if arch["down_attn"][lv]:
                h = R.transformer_2d(P, f"down_blocks.{lv}.attentions.{r}", h, ctx, arch["heads"][lv], arch["transformer_layers"][lv],
                                     arch["linear_proj"], store, f"down-level{lv}-repeat{r}-vit", want_map)
            skips.append(h)
        if lv != L - 1:
            h = R.downsample(P, f"down_blocks.{lv}.downsamplers.0", h, store, f"down-level{lv}-downsampler")
            skips.append(h)
    is_controlnet = down_res is not None and mid_res is not None                                     # :1194
    if is_controlnet:                                                                                # :1236-1245
        assert len(down_res) == len(skips)
        skips = [R._stream(s + r.float()) for s, r in zip(skips, down_res)]

    h = R.resnet_block(P, "mid_block.resnets.0", h, emb, store, "mid-repeat0-res")
    h = R.transformer_2d(P, "mid_block.attentions.0", h, ctx, arch["heads"][-1], arch["transformer_layers"][-1], arch["linear_proj"], store,
                         "mid-vit", want_map)
    h = R.resnet_block(P, "mid_block.resnets.1", h, emb, store, "mid-repeat1-res")
    if is_controlnet:                                                                                # :1269-1270
        h = R._stream(h + mid_res.float())

    for i in range(L):
        lv = L - 1 - i
        for r in range(nl + 1):
            h = torch.cat([h, skips.pop()], dim=1)
            h = R.resnet_block(P, f"up_blocks.{i}.resnets.{r}", h, emb, store, f"up-level{i}-repeat{r}-res")
            if arch["down_attn"][lv]:
                h = R.transformer_2d(P, f"up_blocks.{i}.attentions.{r}", h, ctx, arch["heads"][lv], arch["transformer_layers"][lv],
                                     arch["linear_proj"], store, f"up-level{i}-repeat{r}-vit", want_map)
        if i != L - 1:
            h = R.upsample(P, f"up_blocks.{i}.upsamplers.0", h, store, f"up-level{i}-upsampler")
    h = F.group_norm(h, 32, P["conv_norm_out.weight"], P["conv_norm_out.bias"], 1e-5)
    h = F.silu(h)
    h = F.conv2d(h, P["conv_out.weight"], P["conv_out.bias"], padding=1)
    store.gather("unet", h, "out")
    return h
