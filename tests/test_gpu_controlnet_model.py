"""The native ControlNet on the GPU (-m gpu): NativeControlNet (gdf_controlnet_forward, include/gdf_control.h) against the CPU oracle
(tests/controlnet_model_oracle.py) on the tiny `xl` and `15` architectures of tests/golden/unet_tiny_residuals_*.npz — 16 x 16 latents, a
128 x 128 control image, the true conditioning-embedding widths (16, 32, 96, 256) — the block layout, the chain into NativeUNet, graph
replay, the diffusers-like call surface and FeatureExtractor(control=...)."""
import ctypes as C
import functools
import types

import pytest
import torch

import controlnet_model_oracle as CM
import controlnet_oracle as CO
from helpers import cfg_from_oracle_arch, rel_l2
from oracle import unet_ref as R
from oracle.operand_floor import fp16_operands
from test_controlnet_cpu import residual_golden

pytestmark = pytest.mark.gpu
TOL, TOL_SPLIT = 2e-3, 6e-4      # tests/test_gpu_controlnet.py / test_gpu_unet.py: shrunken widths (with 1.3 x the fp16-operand floor + 5e-5), full split
GUARD = 128                      # sentinel elements (256 bytes) in front of and behind the block: keeps it 256-byte aligned
SENT = -3.0


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """architecture, UNet + ControlNet weights, inputs, control image; the oracle's residuals with and without the fp16-operand rounding and
    the hooks of the UNet oracle fed with them — computed once per architecture and shared, never modified"""
    meta, I, *_ = residual_golden(tag)
    arch = meta["arch"]
    P = CM.synth_controlnet_params(arch, seed=meta["wseed"])
    U = R.synth_params(arch, seed=meta["wseed"])
    cond = CM.synth_cond(meta["batch"], meta["lat"])
    args = (arch, I["sample"], I["timestep"], I["ctx"], I.get("text_embeds"), I.get("time_ids"))

    def run():
        with torch.no_grad():
            down, mid = CM.controlnet_forward(P, *args, cond)
            st = R.Store(None)
            CO.unet_forward_res(U, *args, down, mid, store=st)
        return down + [mid], st.feats
    ref, ref_hooks = run()
    with fp16_operands():
        flo, flo_hooks = run()
    floors = [rel_l2(a, b) for a, b in zip(flo, ref)]
    assert max(floors) < TOL / 1.3, floors          # the 2e-3 cap is a condition on the seeds: every tensor's floor alone leaves it room
    return arch, P, U, I, cond, ref, flo, ref_hooks, flo_hooks


def _cn(arch, P):
    from components.native import NativeControlNet
    cn = NativeControlNet(cfg_from_oracle_arch(arch), device="cuda:0")
    cn.load_state_dict({k: v.half() for k, v in P.items()})
    return cn


def _unet(arch, U, **kw):
    from components.native import NativeUNet
    u = NativeUNet(cfg_from_oracle_arch(arch), device="cuda:0", **kw)
    u.load_state_dict({k: v.half() for k, v in U.items()})
    return u


def _block(cn, I, cond, **kw):
    g = lambda k: I[k].cuda() if k in I else None
    b = cn.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), cond.cuda().half(), **kw)
    torch.cuda.synchronize()
    return b


def _tensors(cn, block, B, lat):
    down, mid = cn.views(block, B, lat, lat)
    return down + [mid]


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_residuals_match_the_oracle(tag):
    """every residual tensor against the oracle: relative L2 < 2e-3 and <= 1.3 x its fp16-operand floor + 5e-5 (plain plan); the block's
    tensors sit at residual_layout's offsets, the bytes between them and the guards around the block are untouched; the second call builds the
    graph, the third builds nothing new and gives equal bits; a float32 control image gives the same bits (8-bit values are exact in fp16)"""
    arch, P, U, I, cond, ref, flo, _, _ = _reference(tag)
    cn = _cn(arch, P)
    B, lat = I["sample"].shape[0], I["sample"].shape[-1]
    lay, nbytes = cn.residual_layout(B, lat, lat)
    assert cn.hook_names() == [] and len(lay) == len(ref)
    buf = torch.full((nbytes // 2 + 2 * GUARD,), SENT, dtype=torch.float16, device="cuda")
    out = buf[GUARD:GUARD + nbytes // 2]
    got = _block(cn, I, cond, out=out)
    assert got is out
    errs = []
    for k, ((off, shape), r, f) in enumerate(zip(lay, ref, flo)):
        assert tuple(r.shape) == shape
        b, c, h, w = shape
        t = out[off // 2:off // 2 + b * c * h * w].view(b, h, w, c).permute(0, 3, 1, 2)
        e, fl = rel_l2(t, r), rel_l2(f, r)
        errs.append(e)
        assert e < TOL and e <= 1.3 * fl + 5e-5, (k, e, fl)
    print(f"[{tag} controlnet] {len(errs)} tensors, worst {max(errs):.2e} (tensor {errs.index(max(errs))})")
    # layout: nothing outside the tensors is written
    used = torch.zeros(nbytes // 2, dtype=torch.bool)
    for off, (b, c, h, w) in lay:
        used[off // 2:off // 2 + b * c * h * w] = True
    assert bool((out.cpu()[~used] == SENT).all()) and bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())
    assert not bool((out.cpu()[used] == SENT).all())
    # deterministic, and replayed from the plan's graph (keyed on the buffer addresses, the output block among them): the second call into the
    # same block builds the graph, the third builds nothing new; the route without out= (a block of the plan's own) gives the same bits
    plan = cn._plan(B, lat, lat, I["ctx"].shape[1], direct=True)
    first = got.clone()
    _block(cn, I, cond, out=out)
    cap = plan.graph_stats()
    b2 = _block(cn, I, cond, out=out).clone()
    assert cap[0] >= 1 and plan.graph_stats() == (cap[0], cap[1] + 1, 0), (cap, plan.graph_stats())
    assert torch.equal(b2, first)
    b1 = _block(cn, I, cond).clone()
    for off, (b, c, h, w) in lay:
        s = slice(off // 2, off // 2 + b * c * h * w)
        assert torch.equal(b1[s], b2[s]) and torch.equal(b1[s], got[s])
    g = lambda k: I[k].cuda() if k in I else None
    b3 = cn.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), cond.cuda().float())
    torch.cuda.synchronize()
    assert all(torch.equal(b3[off // 2:off // 2 + b * c * h * w], b1[off // 2:off // 2 + b * c * h * w]) for off, (b, c, h, w) in lay)


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_residuals_full_split_plan(tag):
    """split = SPLIT_ALL: every operand class of the down / mid program a (hi, lo) pair (the embedding stays plain fp16): < 6e-4 per tensor"""
    from components.native import SPLIT_ALL
    arch, P, U, I, cond, ref, _, _, _ = _reference(tag)
    cn = _cn(arch, P)
    B, lat = I["sample"].shape[0], I["sample"].shape[-1]
    errs = [rel_l2(t, r) for t, r in zip(_tensors(cn, _block(cn, I, cond, split=SPLIT_ALL), B, lat), ref)]
    print(f"[{tag} controlnet, full split] worst {max(errs):.2e}")
    assert max(errs) < TOL_SPLIT, errs


@pytest.mark.parametrize("tag", ["xl", "15"])
def test_chain_into_the_unet(tag):
    """NativeControlNet -> NativeUNet.forward_raw(residuals=block): every hook against unet_forward_res(..., *oracle residuals) within the
    same bounds; the diffusers-like surface (NCHW views into NativeUNet.__call__) gives the bits of the block route"""
    arch, P, U, I, cond, ref, flo, ref_hooks, flo_hooks = _reference(tag)
    cn, u = _cn(arch, P), _unet(arch, U, precise=False)
    B, lat = I["sample"].shape[0], I["sample"].shape[-1]
    g = lambda k: I[k].cuda() if k in I else None
    ids = list(ref_hooks.keys())
    # straight into the UNet plan's staged residual buffer: no staging copy
    dst = u.residual_buffer(B, lat, lat, I["ctx"].shape[1], ids)
    block = _block(cn, I, cond, out=dst)
    noise, hooks = u.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), hook_ids=ids, residuals=block)
    torch.cuda.synchronize()
    assert u._plan(B, lat, lat, I["ctx"].shape[1], ids, False, 0, residuals=True).staged["res"] is dst
    errs = {k: rel_l2(hooks[k], ref_hooks[k]) for k in ids}
    worst = max(errs, key=errs.get)
    print(f"[{tag} controlnet -> unet] hooks={len(ids)} worst {worst} = {errs[worst]:.2e}")
    bad = {k: (v, rel_l2(flo_hooks[k], ref_hooks[k])) for k, v in errs.items() if not (v < TOL and v <= 1.3 * rel_l2(flo_hooks[k], ref_hooks[k]) + 5e-5)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]
    # any other tensor holding the same block: same bits (it is staged by a copy)
    noise2, hooks2 = u.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), hook_ids=ids, residuals=block.clone())
    torch.cuda.synchronize()
    assert torch.equal(noise2, noise) and all(torch.equal(hooks2[k], hooks[k]) for k in ids)

    # __call__ mirrors diffusers: (list of NCHW tensors, mid) that NativeUNet.__call__ and the reference's merge loop take unchanged
    akw = {"text_embeds": g("text_embeds"), "time_ids": g("time_ids")} if "text_embeds" in I else {}
    down, mid = cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half(), conditioning_scale=1,
                   guess_mode=False, added_cond_kwargs=akw, return_dict=False)
    lay = cn.residual_layout(B, lat, lat)[0]
    assert [tuple(t.shape) for t in down + [mid]] == [s for _, s in lay]
    sub = ["mid-repeat1-res-out", "up-level0-repeat0-res-out", ids[-2]]
    seen = {}
    u.feature_store = types.SimpleNamespace(accept_all=False, to_store={k: True for k in sub}, store=lambda t, hid: seen.__setitem__(hid, t))
    out = u(g("sample"), g("timestep"), g("ctx"), added_cond_kwargs=akw, down_block_additional_residuals=down, mid_block_additional_residual=mid,
            return_dict=False)[0]
    # (the same hook set through the block route: a plan without '-map' ids runs its attention on another kernel than the all-hooks plan above)
    noise_s, hooks_s = u.forward_raw(g("sample"), g("timestep"), g("ctx"), g("text_embeds"), g("time_ids"), hook_ids=sub, residuals=block)
    torch.cuda.synchronize()
    assert torch.equal(out, noise_s) and list(seen) == sub and all(torch.equal(seen[k], hooks_s[k]) for k in sub)
    # refusals
    with pytest.raises(NotImplementedError):
        cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half(), conditioning_scale=0.5, added_cond_kwargs=akw)
    with pytest.raises(NotImplementedError):
        cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half(), guess_mode=True, added_cond_kwargs=akw)
    with pytest.raises(ValueError, match="controlnet_cond"):
        cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half()[:, :, :64], added_cond_kwargs=akw)
    with pytest.raises(ValueError, match="controlnet_cond"):
        cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=None, added_cond_kwargs=akw)
    if tag == "xl":
        with pytest.raises(ValueError, match="added_cond_kwargs"):
            cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half())
        with pytest.raises(ValueError, match="text_embeds"):
            cn(g("sample"), g("timestep"), encoder_hidden_states=g("ctx"), controlnet_cond=cond.cuda().half(),
               added_cond_kwargs={"text_embeds": akw["text_embeds"][:, :8], "time_ids": akw["time_ids"]})
    with pytest.raises(ValueError, match="out must be"):
        _block(cn, I, cond, out=torch.zeros(64, dtype=torch.float16, device="cuda"))


def test_plans_refuse_each_others_entry_points():
    """a UNet plan handed to gdf_controlnet_forward, a ControlNet plan handed to gdf_forward / gdf_forward_res, a ControlNet model handed to
    gdf_plan_create: an error with a message, nothing runs"""
    arch, P, U, I, cond, *_ = _reference("15")
    cn, u = _cn(arch, P), _unet(arch, U, precise=False)
    L = cn.lib
    buf = torch.zeros(1 << 20, dtype=torch.float16, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    up = u._plan(1, 16, 16, 77, [], False, 0)
    cp = cn._plan(1, 16, 16, 77)
    assert L.gdf_controlnet_forward(up.handle, p, p, p, None, None, p, 0, p, p, None) != 0 and b"gdf_controlnet_plan_create" in L.gdf_last_error()
    assert L.gdf_forward(cp.handle, p, p, p, None, None, None, p, p, None) != 0 and b"gdf_controlnet_forward" in L.gdf_last_error()
    assert L.gdf_forward_res(cp.handle, p, p, p, None, None, p, None, p, p, None) != 0 and b"gdf_controlnet_forward" in L.gdf_last_error()
    h = C.c_void_p()
    assert L.gdf_plan_create(cn.handle, 1, 16, 16, 77, None, 0, None, C.byref(h)) != 0 and b"gdf_controlnet_plan_create" in L.gdf_last_error()
    assert L.gdf_controlnet_plan_create(u.handle, 1, 16, 16, 77, None, C.byref(h)) != 0 and b"gdf_controlnet_create" in L.gdf_last_error()
    assert L.gdf_controlnet_forward(cp.handle, p, p, p, None, None, p, 7, p, p, None) != 0 and b"GDF_F16 or GDF_F32" in L.gdf_last_error()
    assert L.gdf_controlnet_forward(cp.handle, p, p, p, None, None, p, 0, C.c_void_p(buf.data_ptr() + 16), p, None) != 0 and b"256-byte" in L.gdf_last_error()
    assert L.gdf_controlnet_residual_bytes(cp.handle) == cn.residual_layout(1, 16, 16)[1] and L.gdf_controlnet_residual_bytes(up.handle) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


def test_native_controlnet_from_a_diffusers_like_module():
    """native_controlnet_from(module): `.config` + `.state_dict()` of anything with ControlNetModel's surface; same bits as load_state_dict"""
    from components.native import native_controlnet_from
    arch, P, U, I, cond, *_ = _reference("xl")

    class Stand(torch.nn.Module):
        def __init__(self, **over):
            super().__init__()
            self.params = torch.nn.ParameterDict({k.replace(".", "|"): torch.nn.Parameter(v.half(), requires_grad=False) for k, v in P.items()})
            self.config = types.SimpleNamespace(**dict(dict(
                in_channels=4, block_out_channels=arch["block_out_channels"],
                down_block_types=tuple("CrossAttnDownBlock2D" if a else "DownBlock2D" for a in arch["down_attn"]),
                attention_head_dim=arch["heads"], transformer_layers_per_block=arch["transformer_layers"], cross_attention_dim=arch["cross_dim"],
                use_linear_projection=arch["linear_proj"], addition_embed_type="text_time", addition_time_embed_dim=arch["addition_time_embed_dim"],
                projection_class_embeddings_input_dim=arch["add_in_dim"], layers_per_block=arch["layers_per_block"],
                conditioning_embedding_out_channels=(16, 32, 96, 256), conditioning_channels=3, global_pool_conditions=False,
                controlnet_conditioning_channel_order="rgb", class_embed_type=None), **over))

        def state_dict(self):
            return {k.replace("|", "."): v.data for k, v in self.params.items()}
    a = native_controlnet_from(Stand(), "cuda:0")
    assert a.cfg == dict(cfg_from_oracle_arch(arch), out_channels=4) and a.cond_channels == (16, 32, 96, 256)
    assert torch.equal(_block(a, I, cond), _block(_cn(arch, P), I, cond))
    for over in (dict(global_pool_conditions=True), dict(controlnet_conditioning_channel_order="bgr"), dict(class_embed_type="timestep")):
        with pytest.raises(ValueError):
            native_controlnet_from(Stand(**over), "cuda:0")


def test_feature_extractor_with_control(monkeypatch):
    """FeatureExtractor(control=['canny']) under GDF_SYNTHETIC_WEIGHTS=1, version 1-5 at 128 x 128: use_control changes the up path and only
    the up path; the result is what control_pipe + pipe.unet.forward_raw(residuals=...) give by hand"""
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    layers = ["down-level1-repeat1-vit-out", "mid-repeat1-res-out", "up-level1-repeat1-vit-block0-cross-q", "up-level3-repeat2-res-out"]
    df = diffusion_feature.FeatureExtractor(layer={k: True for k in layers}, version="1-5", img_size=128, device="cuda:0", control=["canny"])
    assert df.control_pipe is not None and len(df.control_pipe.control) == 1
    prompt = df.encode_prompt("a photo of a cat")
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 4, 16, 16, generator=g).half()
    cimg = (torch.randint(0, 256, (2, 3, 128, 128), generator=g).float() / 255)
    keep = lambda f: {k: v.clone() for k, v in f.items()}
    plain = keep(df.extract(prompt, batch_size=2, image=lat, image_type="latents", t=50))
    ctl = keep(df.extract(prompt, batch_size=2, image=lat, image_type="latents", t=50, use_control=True, control_image=cimg))
    again = keep(df.extract(prompt, batch_size=2, image=lat, image_type="latents", t=50, use_control=True, control_image=cimg))
    assert list(ctl) == list(plain) == layers
    for k in layers:
        assert ctl[k].dtype == torch.float16 and bool(torch.isfinite(ctl[k].float()).all())
        assert torch.equal(ctl[k], plain[k]) == (not k.startswith("up-")), k
        assert torch.equal(ctl[k], again[k]), k
    # by hand
    pipe, unet = df.pipe, df.pipe.unet
    ctx = prompt[0].repeat(2, 1, 1).cuda()
    tt = torch.tensor([float(unet_timestep(df, 50))])
    x = pipe.scheduler.scale_model_input(lat.cuda(), tt)
    block = df.control_pipe.generate_control_info(None, x, tt, ctx, {}, control_image=cimg, shared_ctx=True, split=unet.split_for(layers, lat=16))
    _, hooks = unet.forward_raw(x, tt, ctx, hook_ids=layers, shared_ctx=True, residuals=block)
    torch.cuda.synchronize()
    for k in layers:
        assert torch.equal(hooks[k], ctl[k]), k
    with pytest.raises(NotImplementedError, match="ControlNet"):
        df.generate(prompt, 1)
    with pytest.raises(ValueError, match="control_image"):
        df.extract(prompt, batch_size=2, image=lat, image_type="latents", t=50, use_control=True)


def unet_timestep(df, t):
    import copy
    sch = copy.deepcopy(df.scheduler_backup)
    sch.set_timesteps(1000, device="cpu")
    df.pipe.scheduler = sch
    return df.pipe.get_timesteps(1000, t / 1000, "cpu")[0][:1].item()
