"""GPU parity of the MMDiT (Flux) path through the C ABI (include/gdf_flux.h, gdf_ops.h):
kernels vs fp32 PyTorch, whole tiny-Flux forward with every hook vs the CPU oracle (oracle/flux_ref.py), and the
committed reference golden (tests/golden/flux_tiny.npz, produced by the reference's own transformer_flux.py).

Element types: compute_dtype="float16" (fp16 MFMA operands) and "bfloat16" (what the reference runs Flux in,
components/models.py:158-169; mfma_*_bf16, bf16 weights / activations); fp32 accumulate / stream, fp16 hooks in both.
Stated tolerance: relative L2 error per hooked tensor <= 2e-3 (fp16) / <= 1.5e-2 (bf16: 8 mantissa bits, 8x the rounding),
against the fp32 oracle run on the SAME (bf16-representable, where bf16) weights and inputs."""
import ast
import os

import numpy as np
import pytest
import torch

from helpers import rel_l2
from oracle import flux_ref as FR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-3
# "bfloat16x2" (round 4): bf16 weights / inputs / output, activation operands as bf16 hi + lo pairs, fp16 attention internals
# "fp8-mx" (round 4, OPT-IN, lower precision than the reference's bf16): the large linears on OCP e4m3 operands (3 mantissa bits: ~3.7e-2 per GEMM)
TOLS = {"float16": 2e-3, "bfloat16": 1.5e-2, "bfloat16x2": 1.5e-3, "fp8-mx": 1.0e-1, "float16s": 2e-3, "auto": 2e-3}
# element type of the checkpoint / inputs handed to the model ('float16s' / 'auto': a bf16 checkpoint, cast to fp16 operands by the library)
TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "bfloat16x2": torch.bfloat16, "fp8-mx": torch.bfloat16, "float16s": torch.bfloat16,
       "auto": torch.bfloat16}


def _ops():
    from ops_binding import P, lib, ok, stream
    return lib(), P, ok, stream


def _region_major(x_txt, x_img):
    """(B,T,C), (B,S,C) -> [B*T + B*S][C]"""
    return torch.cat([x_txt.reshape(-1, x_txt.shape[-1]), x_img.reshape(-1, x_img.shape[-1])], 0).contiguous()


@pytest.mark.parametrize("M,N,K,variant", [(300, 256, 192, 128), (1024, 512, 256, 1256), (700, 768, 1280, 1256), (520, 64, 256, 128),
                                            # 8-phase main loop: 1, 3 and 20 K-tiles, ragged M / N tiles
                                            (512, 512, 64, 8256), (700, 768, 192, 8256), (1030, 520, 1280, 8256), (4096, 1024, 3072, 8256),
                                            # persistent form: 18 x 18 = 324 tiles walked by 256 workgroups (68 take a second tile), ragged M
                                            (4500, 4608, 192, 8256)])
@pytest.mark.parametrize("mode", ["plain", "gelu", "gate_res", "gate_res_seg"])
@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_gemm_dit(M, N, K, variant, mode, dt):
    L, P, ok, stream = _ops()
    tdt = TDT[dt]
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda", generator=g).to(tdt)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(tdt)
    bias = torch.randn(N, device="cuda", generator=g)
    ref = A.float() @ W.float().t() + bias
    o16 = torch.empty(M, N, device="cuda", dtype=tdt)
    otol = 1e-3 if dt == "float16" else 4e-3                    # 16-bit outputs: rounding of the result itself
    ok(L.gdf_op_set_e16(0 if dt == "float16" else 2), L)
    try:
        _gemm_dit_body(L, P, ok, stream, A, W, bias, ref, o16, M, N, K, variant, mode, g, otol)
    finally:
        L.gdf_op_set_e16(0)


def _gemm_dit_body(L, P, ok, stream, A, W, bias, ref, o16, M, N, K, variant, mode, g, otol):
    if mode == "plain":
        ok(L.gdf_op_gemm_dit(P(A), K, P(W), P(bias), 0, None, 0, 0, 1, 0, 1, None, 0, None, 0, P(o16), N, None, 0, M, N, K, variant, stream()), L)
        got = o16
    elif mode == "gelu":
        ok(L.gdf_op_gemm_dit(P(A), K, P(W), P(bias), 1, None, 0, 0, 1, 0, 1, None, 0, None, 0, P(o16), N, None, 0, M, N, K, variant, stream()), L)
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
        got = o16
    else:
        seg = mode.endswith("seg")
        rps, seg_rows, rps2 = (50, 200, 100) if seg else (100, 0, 1)
        rows = torch.arange(M, device="cuda")
        smp = torch.where(rows < seg_rows, rows // rps, (rows - seg_rows) // rps2) if seg else rows // rps
        nb = int(smp.max()) + 1
        vec = torch.randn(nb, N + 8, device="cuda", generator=g)
        res = torch.randn(M, N, device="cuda", generator=g)
        aux = torch.empty(M, N, device="cuda", dtype=torch.half)
        o32 = res.clone()
        ok(L.gdf_op_gemm_dit(P(A), K, P(W), P(bias), 0, P(vec), N + 8, 1, rps, seg_rows, rps2, P(o32), N, P(aux), N, None, 0,
                             P(o32), N, M, N, K, variant, stream()), L)
        assert rel_l2(aux, ref) < 1e-3                    # pre-gate projection (`attn-out` hook): fp16 in either mode
        ref = res + vec[smp, :N] * ref
        got = o32
        otol = 1e-3                                       # fp32 output: only the operand rounding is left
    torch.cuda.synchronize()
    assert rel_l2(got, ref) < otol, (mode, rel_l2(got, ref))


@pytest.mark.parametrize("M,K,N,silu,acc", [(8, 3072, 70000, 0, 0), (3, 512, 65536 + 37, 1, 1), (8, 256, 1000, 1, 0), (2, 3072, 4096, 0, 1),
                                            (16, 1280, 18000, 1, 0), (12, 320, 5000 + 3, 1, 1), (16, 2816, 1280, 0, 0), (4, 64, 1023, 1, 0)])     # more than 8 rows: one launch per 8
def test_small_linear_both_kernels(M, K, N, silu, acc):
    """N >= 1024 takes the LDS-staged wide kernel (stacked adaLN modulation / time_emb_proj), smaller N the column-per-wave kernel."""
    L, P, ok, stream = _ops()
    g = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(M, K + 8, device="cuda", generator=g)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    bias = torch.randn(N, device="cuda", generator=g)
    out0 = torch.randn(M, N, device="cuda", generator=g)
    out = out0.clone()
    ok(L.gdf_op_small_linear(P(x), K + 8, M, K, P(W), P(bias), N, silu, acc, P(out), N, stream()), L)
    xin = x[:, :K]
    ref = (torch.nn.functional.silu(xin) if silu else xin).double() @ W.double().t() + bias.double() + (out0.double() if acc else 0)
    assert rel_l2(out, ref) < 1e-5


@pytest.mark.parametrize("C", [256, 1024, 3072])
def test_layernorm_mod(C):
    L, P, ok, stream = _ops()
    T, S, B = 8, 24, 3
    R = B * (T + S)
    x = torch.randn(R, C, device="cuda") * 3 + 0.5
    mod = torch.randn(B, 2 * C + 16, device="cuda")
    y = torch.empty(R, C, device="cuda", dtype=torch.half)
    ok(L.gdf_op_layernorm_mod(P(x), C, R, C, 1e-6, P(mod[:, C:]), P(mod), mod.shape[1], T, B * T, S, P(y), stream()), L)
    rows = torch.arange(R, device="cuda")
    smp = torch.where(rows < B * T, rows // T, (rows - B * T) // S)
    ref = torch.nn.functional.layer_norm(x, (C,), eps=1e-6) * (1 + mod[smp, C:2 * C]) + mod[smp, :C]
    assert rel_l2(y, ref) < 1e-3


def test_rope_table_and_qk_norm_rope():
    L, P, ok, stream = _ops()
    T, gh = 8, 4
    S = gh * gh
    ids = torch.cat([torch.zeros(T, 3), FR.latent_image_ids(gh, gh)], 0).cuda()
    cos = torch.empty(T + S, 128, device="cuda"); sin = torch.empty_like(cos)
    ok(L.gdf_op_rope_table(P(ids[:T].contiguous()), T, 16, 56, 56, P(cos), P(sin), 0, stream()), L)
    ok(L.gdf_op_rope_table(P(ids[T:].contiguous()), S, 16, 56, 56, P(cos), P(sin), T, stream()), L)
    rc, rs = FR.rope_freqs(ids.cpu(), (16, 56, 56))
    assert torch.allclose(cos.cpu(), rc, atol=1e-6) and torch.allclose(sin.cpu(), rs, atol=1e-6)
    B, heads, C = 2, 3, 384
    x = torch.randn(B * S, 3 * C, device="cuda").half()
    wq = 1 + 0.1 * torch.randn(128, device="cuda"); wk = 1 + 0.1 * torch.randn(128, device="cuda")
    y = x.clone()
    ok(L.gdf_op_qk_norm_rope(P(y), 3 * C, B * S, heads, 0, C, P(wq), P(wk), 1e-6, P(cos), P(sin), T, S, stream()), L)
    xf = x.float().cpu().view(B, S, 3, heads, 128)
    for which, w in ((0, wq), (1, wk)):
        t = xf[:, :, which].permute(0, 2, 1, 3)                       # B, heads, S, D
        ref = FR.apply_rope(FR.rms_norm(t, w.cpu()), rc[T:], rs[T:]).permute(0, 2, 1, 3).reshape(B * S, C)
        assert rel_l2(y[:, which * C:(which + 1) * C], ref) < 1e-3
    assert torch.equal(y[:, 2 * C:], x[:, 2 * C:])                    # v untouched


@pytest.mark.parametrize("B,heads,T,S", [(2, 2, 64, 256), (1, 3, 40, 100), (2, 1, 8, 16)])
def test_joint_attention(B, heads, T, S):
    L, P, ok, stream = _ops()
    D, C = 128, heads * 128
    g = torch.Generator(device="cuda").manual_seed(7)
    qkv_t = torch.randn(B, T, 3 * C, device="cuda", generator=g).half()
    qkv_i = torch.randn(B, S, 3 * C, device="cuda", generator=g).half()
    buf = _region_major(qkv_t, qkv_i)
    o = torch.zeros(B * (T + S), C, device="cuda", dtype=torch.half)
    base = buf.data_ptr()
    import ctypes
    ptr = lambda col: ctypes.c_void_p(base + col * 2)
    ok(L.gdf_op_attention_joint(ptr(0), 3 * C, ptr(C), 3 * C, ptr(2 * C), 3 * C, P(o), C, B, heads, T, S, D, stream()), L)
    j = torch.cat([qkv_t, qkv_i], 1).float()                          # per-sample joint sequence (B, T+S, 3C)
    q, k, v = [j[..., i * C:(i + 1) * C].view(B, T + S, heads, D).transpose(1, 2) for i in range(3)]
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T + S, C)
    got = torch.cat([o[:B * T].view(B, T, C), o[B * T:].view(B, S, C)], 1)
    assert rel_l2(got, ref) < 2e-3
    # bf16 leg: the same values rounded to bf16 (three fewer mantissa bits: the fp16 bound x 8), reference on those rounded values
    qkv_tb, qkv_ib = qkv_t.float().bfloat16(), qkv_i.float().bfloat16()
    bufb = _region_major(qkv_tb, qkv_ib)
    ob = torch.zeros(B * (T + S), C, device="cuda", dtype=torch.bfloat16)
    baseb = bufb.data_ptr()
    ptrb = lambda col: ctypes.c_void_p(baseb + col * 2)
    ok(L.gdf_op_set_e16(2), L)
    try:
        ok(L.gdf_op_attention_joint(ptrb(0), 3 * C, ptrb(C), 3 * C, ptrb(2 * C), 3 * C, P(ob), C, B, heads, T, S, D, stream()), L)
        torch.cuda.synchronize()
    finally:
        L.gdf_op_set_e16(0)
    jb = torch.cat([qkv_tb, qkv_ib], 1).float()
    q, k, v = [jb[..., i * C:(i + 1) * C].view(B, T + S, heads, D).transpose(1, 2) for i in range(3)]
    refb = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T + S, C)
    gotb = torch.cat([ob[:B * T].view(B, T, C), ob[B * T:].view(B, S, C)], 1)
    assert rel_l2(gotb, refb) < 1.6e-2


def _round(P, I, dt):
    """weights / 16-bit inputs as the model of element type `dt` sees them (the oracle runs on the SAME rounded values)"""
    t = TDT[dt]
    P2 = {k: v.to(t).float() for k, v in P.items()}
    I2 = {k: (v.to(t).float() if k in ("hidden_states", "encoder_hidden_states", "pooled_projections") else v) for k, v in I.items()}
    return P2, I2


def _run_native(arch, P, I, ids, grid, dt="float16"):
    from components.native import NativeFluxTransformer
    cfg = dict(arch)
    net = NativeFluxTransformer(cfg, device="cuda:0", compute_dtype=dt)
    net.load_state_dict({k: v.to(TDT[dt]) for k, v in P.items()})
    assert net.ready()
    out, hooks = net.forward_raw(I["hidden_states"].cuda(), I["encoder_hidden_states"].cuda(), I["pooled_projections"].cuda(),
                                 I["timestep"].cuda(), I["img_ids"].cuda(), I["txt_ids"].cuda(),
                                 guidance=I["guidance"].cuda() if I.get("guidance") is not None else None, hook_ids=ids,
                                 grid=(grid, grid))
    torch.cuda.synchronize()
    return net, out, hooks


@pytest.mark.parametrize("dt", ["float16", "bfloat16", "bfloat16x2", "float16s"])
def test_flux_tiny_all_hooks_vs_oracle(dt):
    arch = FR.tiny_arch()
    P = FR.synth_params(arch, seed=0)
    I = FR.synth_inputs(arch, batch=2, grid=8, n_txt=24, seed=1, same_prompt=False)
    P, I = _round(P, I, dt)
    TOL = TOLS[dt]
    st = FR.Store(None)                                    # accept-all: the eager processor with `*-map` hooks, like the reference
    y = FR.flux_forward(P, arch, I["hidden_states"], I["encoder_hidden_states"], I["pooled_projections"], I["timestep"],
                        I["img_ids"], I["txt_ids"], I["guidance"], store=st)
    net, out, hooks = _run_native(arch, P, I, FR.hook_ids(arch, maps=True), 8, dt)
    assert net.hook_names() == FR.hook_ids(arch, maps=True)
    assert out.dtype == net.io_dtype == (torch.float16 if dt in ('float16', 'float16s', 'auto') else torch.bfloat16)
    assert hooks["vit-block0-cross-map"].shape == (2, 2, 64, 24) and hooks["vit-block3-self-map"].shape == (2, 2, 64, 64)
    assert list(hooks.keys()) == list(st.feats.keys())
    worst = rel_l2(out, y)
    assert worst < (4e-3 if dt == "bfloat16x2" else TOL), ("output", worst)      # (x2: the model OUTPUT is a bf16 tensor: 8 mantissa bits of storage)
    worst = 0.0 if dt == "bfloat16x2" else worst
    for k, ref in st.feats.items():
        assert hooks[k].shape == ref.shape and hooks[k].dtype == torch.float16, k
        e = rel_l2(hooks[k], ref)
        worst = max(worst, e)
        assert e < TOL, (k, e)
    print(f"flux tiny [{dt}]: worst rel L2", worst)


@pytest.mark.parametrize("dt", ["float16", "bfloat16", "bfloat16x2", "fp8-mx"])
def test_flux_fused_qk_norm_rope_epilogue(dt):
    """Blocks without a requested pre-norm q / k / v hook take RMSNorm + RoPE inside the QKV GEMM epilogue; that needs the
    256x256 tile, i.e. a mid-size model: 8 heads x 128, 3 x (1024 + 1024) tokens, 1 double + 1 single block."""
    arch = FR.tiny_arch(heads=8, num_layers=1, num_single_layers=1, joint_dim=256, pooled_dim=64)
    P = FR.synth_params(arch, seed=2)
    I = FR.synth_inputs(arch, batch=3, grid=32, n_txt=1024, seed=3, same_prompt=False)
    P, I = _round(P, I, dt)
    TOL = TOLS[dt]
    st = FR.Store(None)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    y = FR.flux_forward(P, arch, I["hidden_states"], I["encoder_hidden_states"], I["pooled_projections"], I["timestep"],
                        I["img_ids"], I["txt_ids"], I["guidance"], store=st, want_map=False)
    ids = [i for i in FR.hook_ids(arch) if not i.endswith(("-q", "-k", "-v"))]
    net, out, hooks = _run_native(arch, P, I, ids, 32, dt)
    assert list(hooks.keys()) == ids
    assert rel_l2(out, y) < (4e-3 if dt == "bfloat16x2" else TOL), rel_l2(out, y)
    if dt == "fp8-mx":                                   # the large linears really ran on the MX-scaled fp8 MFMA kernel; no fused RMSNorm + RoPE there
        _, _, prof8 = net.forward_raw(I["hidden_states"].cuda(), I["encoder_hidden_states"].cuda(), I["pooled_projections"].cuda(),
                                      I["timestep"].cuda(), I["img_ids"].cuda(), I["txt_ids"].cuda(), guidance=I["guidance"].cuda(),
                                      hook_ids=ids, grid=(32, 32), profile=True)
        kern = {r[0]: r[3] for r in prof8}
        assert kern["attn_qkv"].startswith("gemm_mx_kernel") and kern["ff_out"].startswith("gemm_mx_kernel") and kern["proj_out"].startswith("gemm_mx_kernel")
        assert "quant_fp8" in kern and "qk_norm_rope" in kern
        errs8 = {k: rel_l2(hooks[k], st.feats[k]) for k in ids}
        print("flux fp8-mx: worst hook", max(errs8, key=errs8.get), max(errs8.values()), "median", sorted(errs8.values())[len(errs8) // 2], "output", rel_l2(out, y))
        assert max(errs8.values()) < TOL and max(errs8.values()) > 5e-3       # fp8's own error level: visibly NOT the bf16 path
        return
    for k in ids:
        assert rel_l2(hooks[k], st.feats[k]) < TOL, (k, rel_l2(hooks[k], st.feats[k]))
    print(f"flux fused qkn [{dt}]: worst hook", max(rel_l2(hooks[k], st.feats[k]) for k in ids), "output", rel_l2(out, y))
    # the fused path really ran: no separate pass is left in the op program of this hook set
    _, _, prof = net.forward_raw(I["hidden_states"].cuda(), I["encoder_hidden_states"].cuda(), I["pooled_projections"].cuda(),
                                 I["timestep"].cuda(), I["img_ids"].cuda(), I["txt_ids"].cuda(), guidance=I["guidance"].cuda(),
                                 hook_ids=ids, grid=(32, 32), profile=True)
    assert "qk_norm_rope" not in [r[0] for r in prof] and "attn_qkv" in [r[0] for r in prof]
    # same model, q/k/v hooked (separate in-place pass): identical within fp16 rounding of q / k
    net2, out2, hooks2 = _run_native(arch, P, I, FR.hook_ids(arch), 32, dt)
    assert rel_l2(out2, out) < (1e-3 if dt == "float16" else 8e-3)          # (both outputs are 16-bit tensors of the model's io type)


def test_flux_matches_reference_golden():
    """tests/golden/flux_tiny.npz = outputs of the reference's own FluxTransformer2DModel (gen_golden_flux.py);
    flux_tiny_maps.npz = the same model on the reference's FluxAttnStoreProcessor (`cross-map` / `self-map` hooks)."""
    z = np.load(os.path.join(GOLD, "flux_tiny.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    arch = meta["arch"]
    P = FR.synth_params(arch, seed=meta["wseed"])
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in:")}
    net, out, hooks = _run_native(arch, P, I, meta["order"], 4)
    assert list(hooks.keys()) == meta["order"]
    assert rel_l2(out, torch.from_numpy(z["out:y"])) < TOL
    for k in meta["order"]:
        e = rel_l2(hooks[k], torch.from_numpy(z["out:hook:" + k]))
        assert e < TOL, (k, e)
    zm = np.load(os.path.join(GOLD, "flux_tiny_maps.npz"))
    mm = ast.literal_eval(str(zm["meta"]))
    net, out, hooks = _run_native(arch, P, I, mm["order"], 4)
    assert list(hooks.keys()) == mm["order"] == net.hook_names()
    assert rel_l2(out, torch.from_numpy(zm["out:y"])) < TOL
    for k in mm["order"]:
        if k.endswith("-map"):
            ref = torch.from_numpy(zm["out:hook:" + k])
            assert hooks[k].shape == ref.shape and rel_l2(hooks[k], ref) < TOL, (k, rel_l2(hooks[k], ref))


def test_flux_subset_early_exit_and_unknown_ids():
    arch = FR.tiny_arch(num_layers=1, num_single_layers=2)
    P = FR.synth_params(arch, seed=2)
    I = FR.synth_inputs(arch, batch=1, grid=4, n_txt=8, seed=3)
    ids = ["vit-block1-attn-out", "vit-block0-ffn-inner", "not-a-layer"]
    st = FR.Store({k: True for k in ids})
    FR.flux_forward(P, arch, I["hidden_states"], I["encoder_hidden_states"], I["pooled_projections"], I["timestep"],
                    I["img_ids"], I["txt_ids"], I["guidance"], store=st)
    net, out, hooks = _run_native(arch, P, I, ids, 4)
    assert list(hooks.keys()) == list(st.feats.keys()) == ["vit-block0-ffn-inner", "vit-block1-attn-out"]
    for k, ref in st.feats.items():
        assert rel_l2(hooks[k], ref) < TOL, k


def test_feature_extractor_api_flux_synthetic():
    """FeatureExtractor(version='flux').extract -> pipe(image, prompt, strength=t/1000, guidance_scale=1)
    (reference diffusion_feature.py:246-254) on the synthetic front end with a tiny MMDiT."""
    import numpy as np
    from PIL import Image
    import diffusion_feature
    from components.feature_extractor import flux_layer_ids
    from components.models import SyntheticFluxPipe
    arch = FR.tiny_arch(num_layers=2, num_single_layers=2)
    pipe = SyntheticFluxPipe("cuda:0", seed=0, cfg=arch, n_txt=16)
    assert pipe.transformer.hook_names() == flux_layer_ids(arch) == FR.hook_ids(arch, maps=True)
    layer = {"vit-block0-out": True, "vit-block1-q": True, "vit-block3-out": True, "vit-block2-attn-out": True, "nope": True}
    df = diffusion_feature.FeatureExtractor(layer=layer, version='flux', img_size=128, device='cuda:0', external_model=pipe)
    img = Image.fromarray((np.random.RandomState(0).rand(90, 70, 3) * 255).astype(np.uint8))
    tr = pipe.transformer
    feats = df.extract("a photo of a cat", batch_size=2, image=[img, img], t=100)     # strength 0.1 -> t_start = int(28 - 2.8) = 25:
    # steps 25..27 remain and ONE is run: the reference's patched pipeline returns after its first transformer call (:804-841)
    assert tr.calls == 1 and pipe.last_call["t_start"] == 25
    assert list(feats.keys()) == ["vit-block0-out", "vit-block1-q", "vit-block2-attn-out", "vit-block3-out"]
    for v in feats.values():
        assert v.shape == (2, 256, 8, 8) and v.dtype == torch.float16 and v.is_cuda and torch.isfinite(v.float()).all()
    # ... and what it stored is that forward's hooks: forward_raw on the same packed latents at sigmas[t_start]
    lc = pipe.last_call
    sig = pipe.sigmas(28, 64)
    assert lc["sigma"] == sig[25] and 0.0 < sig[27] < sig[25] < sig[0] == 1.0
    _, hooks = tr.forward_raw(lc["hidden_states"], lc["encoder_hidden_states"], lc["pooled_projections"],
                              torch.full((2,), lc["sigma"], device="cuda:0"), lc["img_ids"], lc["txt_ids"], guidance=lc["guidance"],
                              hook_ids=list(feats.keys()), grid=lc["grid"])
    for k in feats:
        assert torch.equal(hooks[k], feats[k]), k
    f1 = df.extract("x", batch_size=1, image=[img], t=10)                                # strength 0.01 -> the last step only
    assert tr.calls == 2 and pipe.last_call["t_start"] == 27
    assert list(f1.keys()) == list(feats.keys()) and f1["vit-block0-out"].shape == (1, 256, 8, 8)
    f0 = df.extract("x", batch_size=1, image=[img], t=1000)                              # strength 1 -> starts at sigma 1 (pure noise)
    assert tr.calls == 3 and pipe.last_call["t_start"] == 0 and pipe.last_call["sigma"] == 1.0 and list(f0.keys()) == list(feats.keys())


def test_feature_extractor_flux_stock_pipeline_is_stopped_after_one_forward():
    """A STOCK (un-patched) diffusers FluxImg2ImgPipeline loops over every remaining step and then decodes; the reference's vendored
    copy returns after the first transformer call (pipeline_flux_img2img.py:841).  With the native transformer swapped in,
    FeatureExtractor.extract reproduces the reference: the transformer raises SingleForwardDone after its first forward and the
    hooks of THAT forward (the noisiest remaining step) are what is returned."""
    import numpy as np
    from PIL import Image
    import diffusion_feature
    from components.models import SyntheticFluxPipe
    arch = FR.tiny_arch(num_layers=1, num_single_layers=1)

    class StockLikePipe(SyntheticFluxPipe):
        returns_after_first_forward = False

        def __call__(self, image=None, prompt=None, strength=0.6, guidance_scale=7.0, **kw):
            self.steps = 0
            sig = self.sigmas(28, 64)
            t_start = int(max(28 - min(28 * strength, 28), 0))
            SyntheticFluxPipe.__call__(self, image=image, prompt=prompt, strength=strength, guidance_scale=guidance_scale)   # step t_start
            lc = self.last_call
            for i in range(t_start + 1, 28):                            # the rest of the stock denoising loop
                self.steps += 1
                self.transformer(hidden_states=lc["hidden_states"], timestep=torch.full((1,), sig[i], device=self.device),
                                 guidance=lc["guidance"], pooled_projections=lc["pooled_projections"],
                                 encoder_hidden_states=lc["encoder_hidden_states"], txt_ids=lc["txt_ids"], img_ids=lc["img_ids"],
                                 return_dict=False, grid=lc["grid"])
            raise AssertionError("the stock loop ran to its end (VAE decode would follow)")

    pipe = StockLikePipe("cuda:0", seed=0, cfg=arch, n_txt=16)
    df = diffusion_feature.FeatureExtractor(layer={"vit-block0-out": True, "vit-block1-out": True}, version='flux', img_size=128,
                                            device='cuda:0', external_model=pipe)
    img = Image.fromarray((np.random.RandomState(0).rand(90, 70, 3) * 255).astype(np.uint8))
    feats = df.extract("a photo of a cat", batch_size=1, image=[img], t=500)            # 14 steps remain in a stock pipeline
    assert pipe.transformer.calls == 1 and pipe.steps == 0 and pipe.transformer.single_forward is False
    lc = pipe.last_call
    assert lc["t_start"] == 14
    _, hooks = pipe.transformer.forward_raw(lc["hidden_states"], lc["encoder_hidden_states"], lc["pooled_projections"],
                                            torch.full((1,), lc["sigma"], device="cuda:0"), lc["img_ids"], lc["txt_ids"],
                                            guidance=lc["guidance"], hook_ids=list(feats.keys()), grid=lc["grid"])
    for k in feats:
        assert torch.equal(hooks[k], feats[k]), k


def test_flux_early_exit_matches_full_run():
    from components.native import NativeFluxTransformer
    arch = FR.tiny_arch(num_layers=2, num_single_layers=3)
    P = FR.synth_params(arch, seed=4)
    I = FR.synth_inputs(arch, batch=2, grid=4, n_txt=8, seed=5)
    ids = ["vit-block1-ffn-inner", "vit-block2-q", "vit-block3-attn-out"]
    outs = []
    for ee in (False, True):
        net = NativeFluxTransformer(arch, device="cuda:0", early_exit=ee)
        net.load_state_dict({k: v.half() for k, v in P.items()})
        _, hooks = net.forward_raw(I["hidden_states"].cuda(), I["encoder_hidden_states"].cuda(), I["pooled_projections"].cuda(),
                                   I["timestep"].cuda(), I["img_ids"].cuda(), I["txt_ids"].cuda(), guidance=I["guidance"].cuda(),
                                   hook_ids=ids, grid=(4, 4))
        torch.cuda.synchronize()
        outs.append((hooks, net.lib.gdf_plan_num_ops(net._plan(2, 4, 4, 8, ids).handle)))
    (full, n_full), (early, n_early) = outs
    assert list(full.keys()) == list(early.keys()) == ids and n_early < n_full
    for k in ids:
        assert torch.equal(full[k], early[k]), k


def test_flux_range_beyond_fp16_bf16_matches_fp16_saturates():
    """Range safety (reference: Flux runs in bf16, components/models.py:158-169, because real FLUX.1-dev activations leave the
    fp16 range).  One MLP of a small MMDiT is scaled so that its hidden activations reach ~1e6 (> 65504):
      * compute_dtype="bfloat16": every hook downstream is finite and matches the fp32 oracle at the bf16 tolerance; the
        hooked out-of-range tensor itself (`ffn-inner`, stored fp16 like the reference's hooks) is SATURATED at +-65504, where
        the reference's `.to(float16)` would hold inf;
      * compute_dtype="float16": the out-of-range activations saturate instead of turning into inf / NaN — every hook stays
        finite (wrong beyond the saturated layer, by construction of the format, but never poisoned)."""
    arch = FR.tiny_arch(num_layers=2, num_single_layers=2)
    P = FR.synth_params(arch, seed=5)
    big = 1.5e5                                    # weights stay fp16-representable (|w| <= 6e4), the K = C products do not
    P["transformer_blocks.0.ff.net.0.proj.weight"] = (P["transformer_blocks.0.ff.net.0.proj.weight"] * big).clamp(-6.0e4, 6.0e4)
    P["transformer_blocks.0.ff.net.2.weight"] = P["transformer_blocks.0.ff.net.2.weight"] / 64.0    # keep the stream inside fp32 comfort
    I = FR.synth_inputs(arch, batch=2, grid=8, n_txt=16, seed=6, same_prompt=False)
    ids = FR.hook_ids(arch)
    Pb, Ib = _round(P, I, "bfloat16")
    st = FR.Store(None, out_dtype=None)
    with torch.no_grad():
        FR.flux_forward(Pb, arch, Ib["hidden_states"], Ib["encoder_hidden_states"], Ib["pooled_projections"], Ib["timestep"],
                        Ib["img_ids"], Ib["txt_ids"], Ib["guidance"], store=st, want_map=False)
    inner = st.feats["vit-block0-ffn-inner"].float()
    assert float(inner.abs().max()) > 65504 * 4                                     # the test really leaves the fp16 range
    net, out, hooks = _run_native(arch, Pb, Ib, ids, 8, "bfloat16")
    for k in ids:
        h = hooks[k].float()
        assert torch.isfinite(h).all(), k
        if k == "vit-block0-ffn-inner":
            assert float(h.abs().max()) == 65504.0                                   # saturated, not inf
            sat = inner.clamp(-65504, 65504)
            assert rel_l2(h, sat) < 2e-2
        elif k not in ("vit-block0-out",):                                            # (block 0 `out` = norm-out: before the big MLP)
            e = rel_l2(h, st.feats[k])
            assert e < 2e-2, (k, e)
    assert torch.isfinite(out.float()).all()
    net16, out16, hooks16 = _run_native(arch, *_round(P, I, "float16"), ids, 8, "float16")
    for k in ids:
        assert torch.isfinite(hooks16[k].float()).all(), k                           # saturated arithmetic, never inf / NaN
    assert torch.isfinite(out16.float()).all()
    # 'float16s' / 'auto' (round 5, the product default): fp16 operands, the MLP hidden tensors stored x 2^-8 — the SAME 1e6 activations stay in
    # range, and every hook downstream matches the fp32 oracle at the fp16 tolerance (plain 'float16' above is wrong beyond the saturated layer)
    nets, outs, hookss = _run_native(arch, Pb, Ib, ids, 8, "auto")
    assert nets.cfg["compute_dtype"] == "auto" and nets.fp16_cast_error <= 1e-4      # the bf16 -> fp16 weight cast was checked and is exact here
    for k in ids:
        h = hookss[k].float()
        assert torch.isfinite(h).all(), k
        if k == "vit-block0-ffn-inner":
            assert float(h.abs().max()) == 65504.0 and rel_l2(h, inner.clamp(-65504, 65504)) < 2e-3     # the fp16 hook itself saturates
        else:
            e = rel_l2(h, st.feats[k])
            assert e < 3e-3, (k, e)
    assert torch.isfinite(outs.float()).all()


def test_flux_float16s_single_block_mlp_beyond_fp16():
    """The single blocks contract over [attn | mlp] rows in ONE GEMM, so under 'float16s' the attention output carries the MLP's 2^-8 range scale
    (AttnParams::o_scale) and the `attn-out` hook undoes it: a single block whose proj_mlp hidden reaches ~1e6 still matches the oracle on
    every hook, and `attn-out` equals the un-scaled attention output."""
    arch = FR.tiny_arch(num_layers=1, num_single_layers=3)
    P = FR.synth_params(arch, seed=7)
    P["single_transformer_blocks.0.proj_mlp.weight"] = (P["single_transformer_blocks.0.proj_mlp.weight"] * 1.5e5).clamp(-6.0e4, 6.0e4)
    w = "single_transformer_blocks.0.proj_out.weight"
    C = arch["num_attention_heads"] * arch["attention_head_dim"]
    P[w] = torch.cat([P[w][:, :C], P[w][:, C:] / 4096.0], 1)                          # keep the stream moderate: only the MLP columns shrink
    I = FR.synth_inputs(arch, batch=2, grid=8, n_txt=16, seed=8, same_prompt=False)
    ids = FR.hook_ids(arch)
    Pb, Ib = _round(P, I, "bfloat16")
    st = FR.Store(None, out_dtype=None)
    with torch.no_grad():
        y = FR.flux_forward(Pb, arch, Ib["hidden_states"], Ib["encoder_hidden_states"], Ib["pooled_projections"], Ib["timestep"],
                            Ib["img_ids"], Ib["txt_ids"], Ib["guidance"], store=st, want_map=False)
    net, out, hooks = _run_native(arch, Pb, Ib, ids, 8, "float16s")
    errs = {k: rel_l2(hooks[k], st.feats[k]) for k in ids}
    worst = max(errs, key=errs.get)
    print(f"[flux float16s, single-block MLP hidden ~1e6] worst {worst} = {errs[worst]:.2e}; output {rel_l2(out, y):.2e}")
    assert errs[worst] < 3e-3, (worst, errs[worst])
    assert rel_l2(out, y) < 3e-3
    # plain float16 on the same model: the saturated hidden tensor corrupts what follows
    _, out16, hooks16 = _run_native(arch, *_round(P, I, "float16"), ids, 8, "float16")
    assert max(rel_l2(hooks16[k], st.feats[k]) for k in ids if k.endswith("-out")) > 1e-2


def test_flux_auto_falls_back_to_bf16x2_when_weights_do_not_survive_fp16():
    """'auto' = 'float16s' guarded at load time: a checkpoint with a weight matrix outside fp16's range (|w| > 65504) or made of values below
    fp16's normal range is loaded as 'bfloat16x2' instead, with one RuntimeWarning — and still matches the oracle."""
    import warnings
    from components.native import NativeFluxTransformer
    arch = FR.tiny_arch(num_layers=1, num_single_layers=1)
    P = FR.synth_params(arch, seed=9)
    I = FR.synth_inputs(arch, batch=1, grid=8, n_txt=16, seed=10)
    k1, k2 = "transformer_blocks.0.ff.net.2.weight", "transformer_blocks.0.ff.net.0.proj.weight"
    P[k1] = P[k1] * 2.0 ** -20                     # every value far below fp16's normal range (6.1e-5): the cast would keep 0-4 mantissa bits
    P[k2] = P[k2] * 2.0 ** 20                      # ... compensated upstream, beyond fp16's range on the way: bf16 holds both exactly
    Pb, Ib = _round(P, I, "bfloat16")
    ids = FR.hook_ids(arch)
    st = FR.Store(None, out_dtype=None)
    with torch.no_grad():
        FR.flux_forward(Pb, arch, Ib["hidden_states"], Ib["encoder_hidden_states"], Ib["pooled_projections"], Ib["timestep"],
                        Ib["img_ids"], Ib["txt_ids"], Ib["guidance"], store=st, want_map=False)
    net = NativeFluxTransformer(dict(arch), device="cuda:0", compute_dtype="auto")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        net.load_state_dict({k: v.to(torch.bfloat16) for k, v in Pb.items()})
    assert [x for x in w if "bfloat16x2" in str(x.message)] and net.cfg["compute_dtype"] == "bfloat16x2" and net.io_dtype == torch.bfloat16
    out, hooks = net.forward_raw(Ib["hidden_states"].cuda(), Ib["encoder_hidden_states"].cuda(), Ib["pooled_projections"].cuda(),
                                 Ib["timestep"].cuda(), Ib["img_ids"].cuda(), Ib["txt_ids"].cuda(), guidance=Ib["guidance"].cuda(),
                                 hook_ids=ids, grid=(8, 8))
    torch.cuda.synchronize()
    for k in ids:
        if k != "vit-block0-ffn-inner":            # (the hooked hidden tensor itself is ~1e6 x: saturated fp16, like the reference's .to(float16) inf)
            assert rel_l2(hooks[k], st.feats[k]) < 3e-3, (k, rel_l2(hooks[k], st.feats[k]))


def test_flux_attention_argument_is_accepted_and_ignored():
    """Reference quirk: FeatureExtractor(version='flux', attention=[...]) registers an AttentionStore, but the flux branch of
    extract() returns before the aggregation step (diffusion_feature.py:246-254 vs :492-500): no 'attn' entry.  Same here."""
    import numpy as np
    from PIL import Image
    import diffusion_feature
    from components.models import SyntheticFluxPipe
    arch = FR.tiny_arch(num_layers=1, num_single_layers=1)
    pipe = SyntheticFluxPipe("cuda:0", seed=0, cfg=arch, n_txt=16)
    df = diffusion_feature.FeatureExtractor(layer={"vit-block0-out": True}, version='flux', img_size=128, device='cuda:0',
                                            external_model=pipe, attention=['up_cross'])
    img = Image.fromarray((np.random.RandomState(0).rand(90, 70, 3) * 255).astype(np.uint8))
    feats = df.extract("a photo of a cat", batch_size=1, image=[img], t=10)
    assert list(feats.keys()) == ["vit-block0-out"]


@pytest.mark.parametrize("M,N,K,mode", [(512, 256, 256, "plain"), (1000, 768, 3072, "gelu"), (4096, 3072, 1024, "res"), (300, 512, 128, "plain")])
def test_fp8_mx_quant_and_gemm(M, N, K, mode):
    """'fp8-mx' building blocks (include/gdf_ops.h): row quantisation to OCP e4m3 with a power-of-two scale per row, and the MX-scaled MFMA
    GEMM on such operands — checked against fp32 arithmetic on the DEQUANTISED operands (what remains is fp32 summation order and the bf16
    rounding of the output), and against the unquantised product at fp8's own tolerance."""
    L, P, ok, stream = _ops()
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = (torch.randn(M, K, device="cuda", generator=g) * torch.rand(M, 1, device="cuda", generator=g) * 8).bfloat16()
    A[::7, 5] *= 30.0                                                  # rows with an outlier
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g)

    def quant(X):
        q = torch.empty(X.shape, dtype=torch.uint8, device="cuda"); sc = torch.empty(X.shape[0], device="cuda")
        ok(L.gdf_op_quant_rows_fp8(P(X), X.shape[1], X.shape[0], X.shape[1], 1, P(q), X.shape[1], P(sc), stream()), L)
        return q, sc
    A8, sa = quant(A)
    W8, sw = quant(W)
    torch.cuda.synchronize()
    # the quantiser: power-of-two scales, |q| <= 448, dequantised values within e4m3's half-ulp (2^-4 relative) of the source
    assert torch.all(torch.frexp(sa)[0] == 0.5) and torch.all(torch.frexp(sw)[0] == 0.5)
    dA = A8.view(torch.float8_e4m3fn).float() * sa[:, None]
    dW = W8.view(torch.float8_e4m3fn).float() * sw[:, None]
    assert float(A8.view(torch.float8_e4m3fn).float().abs().max()) <= 448.0
    amax = A.float().abs().amax(1, keepdim=True)
    # |err| <= half an ulp of the top binade (e4m3: 3 mantissa bits; the scaled row maximum lies in (224, 448], ulp there = 32)
    assert float(((dA - A.float()).abs() / amax).max()) <= 16.0 / 224.0 + 1e-6
    assert rel_l2(dA, A.float()) < 4e-2 and rel_l2(dW, W.float()) < 4e-2
    o16 = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    o32 = torch.empty(M, N, device="cuda") if mode == "res" else None
    res = torch.randn(M, N, device="cuda", generator=g) if mode == "res" else None
    ok(L.gdf_op_gemm_mx(P(A8), K, P(sa), P(W8), P(sw), P(bias), 1 if mode == "gelu" else 0, P(res), N, P(o16), N, P(o32), N, M, N, K, stream()), L)
    torch.cuda.synchronize()
    ref = dA @ dW.t() + bias
    if mode == "gelu":
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if mode == "res":
        ref = ref + res
        assert rel_l2(o32, ref) < 2e-6 * K ** 0.5 + 1e-5, rel_l2(o32, ref)          # fp32 accumulation of exact fp8 products
    assert rel_l2(o16, ref) < 3e-3, rel_l2(o16, ref)                                 # + the bf16 rounding of the output
    full = A.float() @ W.float().t() + bias
    if mode == "gelu":
        full = torch.nn.functional.gelu(full, approximate="tanh")
    if mode == "res":
        full = full + res
    e = rel_l2(o16, full)
    print(f"fp8-mx gemm {M}x{N}x{K} {mode}: vs dequantised {rel_l2(o16, ref):.2e}, vs unquantised {e:.2e}")
    assert e < 6e-2
