"""The native ControlNet without a GPU: exported and bound symbols, the parameter table libgdf.so registers against the oracle's state dict
(tests/controlnet_model_oracle.py), the oracle's self-consistency with the residual-injected UNet oracle, the host logic of
components/control.py with a stub model, and the CLI flag."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import controlnet_model_oracle as CM
import controlnet_oracle as CO
from helpers import cfg_from_oracle_arch
from oracle import unet_ref as R
from test_controlnet_cpu import residual_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gdf_controlnet_create", "gdf_controlnet_layout", "gdf_controlnet_plan_create", "gdf_controlnet_forward", "gdf_controlnet_residual_bytes")
NEW_OPS = ("gdf_op_cond_conv3x3", "gdf_op_cond_weight_bytes", "gdf_op_cond_pack_weights", "gdf_op_cond_pack_image")


def test_symbols_are_exported_declared_and_bound():
    from components import native
    L = native.load_library()
    hdr = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("gdf.h", "gdf_control.h", "gdf_ops.h")}
    for n in NEW:
        assert hasattr(L, n) and n in native.SIGNATURES and n + "(" in hdr["gdf.h"] and n + "(" in hdr["gdf_control.h"], n
    for n in NEW_OPS:
        assert hasattr(L, n) and n + "(" in hdr["gdf_ops.h"], n
    assert L.gdf_abi_version() == 1
    import __graft_entry__ as G
    assert "cond_embed.hip" in G.SOURCES


def test_null_and_foreign_plans_are_refused_by_message():
    from components import native
    L = native.load_library()
    z = C.c_void_p(0)
    assert L.gdf_controlnet_forward(z, z, z, z, z, z, z, 0, z, z, z) != 0 and b"null plan" in L.gdf_last_error()
    h = C.c_void_p()
    assert L.gdf_controlnet_plan_create(z, 1, 16, 16, 77, None, C.byref(h)) != 0 and b"null" in L.gdf_last_error()
    assert L.gdf_controlnet_residual_bytes(z) == 0
    a = native.arch_desc(native.ARCH_CONFIGS["1-5"])
    cc = (C.c_int * 4)(16, 32, 96, 256)
    if not torch.cuda.is_available():
        assert L.gdf_controlnet_create(C.byref(a), C.byref(cc), 3, C.byref(h)) != 0 and b"no HIP device" in L.gdf_last_error()
    bad = (C.c_int * 4)(16, 32, 64, 128)
    assert L.gdf_controlnet_layout(C.byref(a), C.byref(bad), 3, C.byref(h)) != 0 and b"(16, 32, 96, 256)" in L.gdf_last_error()
    # a parameter table has no weights: it takes no parameter and builds no plan
    assert L.gdf_controlnet_layout(C.byref(a), C.byref(cc), 3, C.byref(h)) == 0
    p = C.c_void_p()
    assert L.gdf_controlnet_plan_create(h, 1, 16, 16, 77, None, C.byref(p)) != 0 and b"without weights" in L.gdf_last_error()
    assert L.gdf_model_set_param(h, b"conv_in.bias", C.c_void_p(64), 0, None) != 0 and b"without weights" in L.gdf_last_error()
    assert L.gdf_model_hook_count(h) == 0 and not L.gdf_model_ready(h)
    L.gdf_model_destroy(h)


def _archs():
    out = [(tag, residual_golden(tag)[0]["arch"]) for tag in ("xl", "15")]
    return out + [("1-5", R.ARCHS["1-5"]), ("sdxl", R.ARCHS["xl"])]


@pytest.mark.parametrize("name,arch", _archs(), ids=[n for n, _ in _archs()])
def test_parameter_table_equals_the_oracle_state_dict(name, arch):
    """names and shapes gdf_controlnet_create registers == diffusers' ControlNetModel state dict as the oracle spells it: the UNet's encoder
    names, the eight embedding convs, one 1x1 conv per skip (12 for the SD1.5 topology, 9 for SDXL's) + 1; no up path, no output head"""
    from components import native
    got = native.controlnet_param_shapes(cfg_from_oracle_arch(arch))
    want = CM.controlnet_param_shapes(arch)
    assert set(got) == set(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert all(tuple(got[k]) == tuple(want[k]) for k in want), [k for k in want if tuple(got[k]) != tuple(want[k])][:5]
    n1x1 = [k for k in got if k.startswith("controlnet_down_blocks.") and k.endswith(".weight")]
    assert len(n1x1) == {3: 9, 4: 12}[len(arch["block_out_channels"])]
    assert got["controlnet_mid_block.weight"] == (arch["block_out_channels"][-1],) * 2 + (1, 1)
    assert not [k for k in got if k.startswith(("up_blocks.", "conv_norm_out.", "conv_out."))]
    assert got["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert got["controlnet_cond_embedding.conv_out.weight"] == (arch["block_out_channels"][0], 256, 3, 3)
    unet = R.param_shapes(arch)
    assert all(tuple(unet[k]) == tuple(v) for k, v in got.items() if k in unet)
    if name in ("xl", "15"):
        P = CM.synth_controlnet_params(arch, seed=0)
        assert list(P) == list(want) and all(tuple(P[k].shape) == tuple(want[k]) for k in want)
        assert all(float(P[k].abs().max()) > 0 for k in P if k.startswith("controlnet_"))            # no zero convs: the tests are not vacuous


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_oracle_feeds_the_residual_oracle(tag):
    """controlnet_forward's outputs have the shapes of down_block_additional_residuals / mid_block_additional_residual and
    unet_forward_res takes them; the conditioning image matters and so does every 1x1 conv"""
    meta, I, *_ = residual_golden(tag)
    arch = meta["arch"]
    P = CM.synth_controlnet_params(arch, seed=meta["wseed"])
    U = R.synth_params(arch, seed=meta["wseed"])
    cond = CM.synth_cond(meta["batch"], meta["lat"])
    args = (arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"))
    with torch.no_grad():
        down, mid = CM.controlnet_forward(P, *args, cond)
        d2, m2 = CM.controlnet_forward(P, *args, 1 - cond)
        y = CO.unet_forward_res(U, *args, down, mid)
        y0 = R.unet_forward(U, *args)
    ds, ms = CO.residual_shapes(arch, meta["batch"], meta["lat"])
    assert [tuple(t.shape) for t in down] == ds and tuple(mid.shape) == ms
    assert tuple(y.shape) == tuple(y0.shape) and not torch.equal(y, y0) and bool(torch.isfinite(y).all())
    assert all(not torch.equal(a, b) for a, b in zip(down + [mid], d2 + [m2]))
    # skip 0 is the 1x1 conv of conv_in(sample) + embedding(cond): the restated wiring, spelled out once
    import torch.nn.functional as F
    with torch.no_grad():
        h0 = F.conv2d(I["sample"], P["conv_in.weight"], P["conv_in.bias"], padding=1) + CM.cond_embedding(P, cond)
        want0 = F.conv2d(h0, P["controlnet_down_blocks.0.weight"], P["controlnet_down_blocks.0.bias"])
    assert tuple(CM.cond_embedding(P, cond).shape) == tuple(h0.shape) and torch.allclose(down[0], want0)


class _Stub:
    """stands in for a NativeControlNet: records its inputs, returns a fixed block"""

    def __init__(self, block):
        self.block, self.calls = block, []

    def forward_raw(self, latents, t, ctx, text_embeds, time_ids, cond, shared_ctx=False, split=0, out=None):
        self.calls.append(dict(cond=cond, shared_ctx=shared_ctx, split=split, out=out, text_embeds=text_embeds))
        if out is not None:
            out.copy_(self.block)
            return out
        return self.block.clone()


def _pipe():
    return types.SimpleNamespace(vae_scale_factor=8, synthetic_weights=True, unet=types.SimpleNamespace(cfg={}))


def test_control_pipeline_host_logic(monkeypatch):
    from PIL import Image
    from components import control as K
    with pytest.raises(NotImplementedError):
        K.ControlNetPipeline(_pipe(), ["canny", "scribble"], "cpu", models=[None, None])
    g = torch.Generator().manual_seed(0)
    a, b = (torch.randn(640, generator=g).half() for _ in range(2))
    sa, sb = _Stub(a), _Stub(b)
    cp = K.ControlNetPipeline(_pipe(), ["canny", "depth"], "cpu", models=[sa, sb])
    lat = torch.zeros(2, 4, 2, 3)
    arr = torch.randint(0, 256, (2, 16, 24, 3), generator=g, dtype=torch.uint8)
    pil = [Image.fromarray(x.numpy()) for x in arr]
    ten = arr.permute(0, 3, 1, 2).float() / 255
    # already-processed control images, tensor and PIL: the same (B, 3, 8 H, 8 W) fp16 tensor in [0, 1], no preprocessor, and the fp16 sum
    out_t = cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {"text_embeds": "te"}, control_image=ten, shared_ctx=True, split=5)
    out_p = cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {}, control_image=pil)
    c_t, c_p = sa.calls[0]["cond"], sa.calls[1]["cond"]
    assert c_t.dtype == torch.float16 and tuple(c_t.shape) == (2, 3, 16, 24) and torch.equal(c_t, c_p) and torch.equal(c_t, ten.half())
    assert 0 <= float(c_t.min()) and float(c_t.max()) <= 1
    assert sa.calls[0]["shared_ctx"] is True and sa.calls[0]["split"] == 5 and sa.calls[0]["text_embeds"] == "te" and sb.calls[0]["split"] == 5
    assert torch.equal(out_t, a + b) and torch.equal(out_p, a + b) and out_t.dtype == torch.float16
    # out=: the first model writes into it, the second is added in place, in fp16
    dst = torch.zeros(640, dtype=torch.float16)
    got = cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {}, control_image=ten, out=dst)
    assert got is dst and torch.equal(dst, a + b) and sa.calls[-1]["out"] is dst and sb.calls[-1]["out"] is None
    # a control image of another size is resized to 8 H x 8 W
    cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {}, control_image=[p.resize((12, 8)) for p in pil])
    assert tuple(sa.calls[-1]["cond"].shape) == (2, 3, 16, 24)
    with pytest.raises(ValueError):
        cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {}, control_image=torch.zeros(2, 4, 16, 24))
    with pytest.raises(ValueError):
        cp.generate_control_info(None, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {})
    # a missing preprocessor module is named, with the way round it
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "controlnet_aux", None)
    one = K.ControlNetPipeline(_pipe(), ["canny"], "cpu", models=[sa])
    with pytest.raises(NotImplementedError, match="cv2.*control_image="):
        one.generate_control_info(pil, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {})
    dep = K.ControlNetPipeline(_pipe(), ["depth"], "cpu", models=[sb])
    with pytest.raises(NotImplementedError, match="controlnet_aux.*control_image="):
        dep.generate_control_info(pil, lat, torch.tensor([1.0]), torch.zeros(2, 7, 8), {})


def test_canny_preprocessor_with_a_stand_in_cv2(monkeypatch):
    """reference controlnet.py:30-36: Canny(image, 100, 200) replicated to three channels, handed on as a PIL image"""
    from PIL import Image
    from components import control as K
    seen = {}

    def canny(img, lo, hi):
        seen["args"] = (img.shape, lo, hi)
        return (img[:, :, 0] > 127).astype(np.uint8) * 255
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(Canny=canny))
    src = Image.fromarray((np.arange(8 * 8 * 3) % 256).astype(np.uint8).reshape(8, 8, 3))
    out = K.canny_preprocessor()(src)
    assert seen["args"] == ((8, 8, 3), 100, 200) and out.size == (8, 8) and out.mode == "RGB"
    e = np.array(out)
    assert np.array_equal(e[:, :, 0], e[:, :, 1]) and np.array_equal(e[:, :, 0], e[:, :, 2]) and set(np.unique(e)) <= {0, 255}
    t = K.control_tensor([out], 8, 8)
    assert set(t.unique().tolist()) <= {0.0, 1.0}


def test_extractor_refusals():
    import diffusion_feature as D
    with pytest.raises(NotImplementedError, match="control="):
        D.FeatureExtractor(None, "flux", "cpu", control=["canny"])
    with pytest.raises(NotImplementedError, match="control="):
        D.FeatureExtractor(None, "pixart-sigma", "cpu", control=["canny"])
    fx = types.SimpleNamespace(version="1-5", control_pipe=object(), attention=None)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        D.FeatureExtractor.generate(fx, None, 1)
    with pytest.raises(NotImplementedError, match="denoising_from"):
        D.FeatureExtractor.extract(fx, None, 1, None, use_control=True, control_image=torch.zeros(1, 3, 8, 8), denoising_from=100)
    with pytest.raises(ValueError, match="control_image"):
        D.FeatureExtractor.extract(fx, None, 1, torch.zeros(1, 3, 8, 8), image_type="tensors", use_control=True)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        D.FeatureExtractor.extract(types.SimpleNamespace(version="1-5", control_pipe=None), None, 1, None, use_control=True)


def test_cli_control_flag_parses():
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    base = ["--version", "1-5", "--t", "50"]

    def parse(extra):
        try:
            return cli.parse_args(base + extra)
        except SystemExit:                       # (other flags the parser requires)
            return cli.parse_args(base + ["--input_dir", "x", "--output_dir", "y"] + extra)
    assert parse([]).control is None
    assert parse(["--control", "canny"]).control == ["canny"]
    assert parse(["--control", "canny", "depth"]).control == ["canny", "depth"]
