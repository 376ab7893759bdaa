"""ControlNet residuals without a GPU: the residual-injected oracle (tests/controlnet_oracle.py) against golden vectors from the reference's
own UNet2DConditionModel.forward (tests/golden/gen_golden_controlnet.py), and the residual block layout libgdf.so computes (include/gdf.h,
gdf_residual_*: host arithmetic) against diffusers' skip order."""
import ast
import os

import numpy as np
import pytest
import torch

import controlnet_oracle as CO
from oracle import unet_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def residual_golden(tag):
    """tests/golden/unet_tiny_residuals_<tag>.npz -> (meta, inputs, down residuals, mid residual, {id: (idx, values, norm, shape)}, out)"""
    z = np.load(os.path.join(GOLD, f"unet_tiny_residuals_{tag}.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in:")}
    down, mid = CO.synth_residuals(meta["arch"], meta["batch"], meta["lat"], seed=meta["res_seed"], scale=meta["res_scale"])
    # the fixture pins the (seeded) residuals by per-tensor checksums
    assert np.allclose([float(t.double().sum()) for t in down + [mid]], z["res_sum"], rtol=0, atol=1e-9)
    assert np.allclose([float(t.double().abs().sum()) for t in down + [mid]], z["res_abs"], rtol=0, atol=1e-9)
    hooks = {}
    for n, k in enumerate(meta["order"]):
        shape = tuple(int(s) for s in z["shape:" + k])
        numel = int(np.prod(shape))
        idx = torch.randint(0, numel, (min(meta["ns"], numel),), generator=torch.Generator().manual_seed(n))
        hooks[k] = (idx, torch.from_numpy(z["hook:" + k]), float(z["norm:" + k]), shape)
    return meta, I, down, mid, hooks, torch.from_numpy(z["out"])


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_residual_oracle_matches_reference_forward(tag):
    """unet_forward_res against the reference's forward with down_block_additional_residuals / mid_block_additional_residual
    (unet_2d_condition.py:1194, 1236-1245, 1269-1270), every hook, at the bound tests/test_oracle_golden.py holds the plain forward to."""
    meta, I, down, mid, hooks, out = residual_golden(tag)
    arch = meta["arch"]
    P = R.synth_params(arch, seed=meta["wseed"])
    st = R.Store(None, out_dtype=None)
    with torch.no_grad():
        y = CO.unet_forward_res(P, arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"), down, mid, store=st,
                                want_map=False)
    assert list(st.feats.keys()) == meta["order"]
    assert torch.allclose(y, out, atol=2e-5, rtol=1e-5)
    for k, (idx, vals, norm, shape) in hooks.items():
        got = st.feats[k].float().contiguous()
        assert tuple(got.shape) == shape, k
        assert torch.allclose(got.flatten()[idx], vals, atol=2e-5, rtol=1e-5), (k, float((got.flatten()[idx] - vals).abs().max()))
        assert abs(float(got.double().norm()) - norm) <= 1e-5 * norm + 1e-6, k


def test_residual_oracle_touches_the_up_path_only():
    """the down and mid hooks of the forward with residuals equal those without, the up hooks and the output do not; no residuals = unet_forward"""
    arch = R.tiny_arch("xl")
    P = R.synth_params(arch, seed=0)
    I = R.synth_inputs(arch, 1, 8, seed=1)
    down, mid = CO.synth_residuals(arch, 1, 8)
    args = (P, arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"))
    a, b, c = R.Store(None, out_dtype=None), R.Store(None, out_dtype=None), R.Store(None, out_dtype=None)
    with torch.no_grad():
        ya = R.unet_forward(*args, store=a, want_map=False)
        yb = CO.unet_forward_res(*args, store=b, want_map=False)
        yc = CO.unet_forward_res(*args, down, mid, store=c, want_map=False)
    assert torch.equal(ya, yb) and all(torch.equal(a.feats[k], b.feats[k]) for k in a.feats)
    for k in a.feats:
        same = torch.equal(a.feats[k], c.feats[k])
        assert same == (not k.startswith("up-") and k != "unet-out"), k
    assert not torch.equal(ya, yc)
    with pytest.raises(AssertionError):
        CO.unet_forward_res(*args, down[:-1], mid)


@pytest.mark.parametrize("version,count", [("1-5", 12), ("2-1", 12), ("xl", 9)])
def test_residual_layout(version, count):
    """gdf_residual_info: diffusers' skip order (conv_in; per level every resnet(+transformer) output, then the downsampler) with the mid
    block's tensor last, true channel widths, 256-byte-aligned offsets that do not overlap, for two batch / latent sizes."""
    from components import native
    cfg = native.ARCH_CONFIGS[version]
    arch = R.ARCHS[version]
    for batch, h, w in ((1, 64, 64), (3, 32, 48)):
        lay, nbytes = native.residual_layout(cfg, batch, h, w)
        down, mid = CO.residual_shapes(arch, batch, h, w)
        assert len(lay) == count + 1 and len(down) == count
        assert [s for _, s in lay] == down + [mid]
        end = 0
        for off, (b, c, hh, ww) in lay:
            assert off % 256 == 0 and off >= end
            end = off + b * c * hh * ww * 2
        assert end <= nbytes and nbytes % 256 == 0 and nbytes - end < 256
    boc = cfg["block_out_channels"]
    assert [s[1] for _, s in native.residual_layout(cfg, 1, 64, 64)[0]] == (
        [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280] if len(boc) == 4 else [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280])


def test_residual_layout_binding_is_declared():
    """the new entry points are part of the header and of the binding table (tests/test_host_cpu.py compares the two sets as wholes)"""
    from components import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdf.h")).read()
    for name in ("gdf_forward_res", "gdf_plan_residual_count", "gdf_plan_residual_info", "gdf_plan_residual_bytes", "gdf_residual_count",
                 "gdf_residual_info", "gdf_residual_bytes"):
        assert name in native.SIGNATURES and name + "(" in hdr, name
    assert native.load_library().gdf_abi_version() == 1
