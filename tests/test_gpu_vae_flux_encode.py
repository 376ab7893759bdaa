"""The native Flux VAE encoder (-m gpu): NativeVAEEncoder.encode_packed (gdf_vae_encode_packed, csrc/vae.cpp) with 16 latent channels and no
quant_conv against the fp32 CPU oracle (oracle/vae_ref.py, parametrised by latent_channels / use_quant_conv), on the two shrunken shapes
tests/test_gpu_vae.py::test_vae_encode_matches_oracle uses and at its tolerance for this encoder at these widths, relative L2 < 3e-3.

Reference: VR.prepare_latents(..., scaling, noise_a = 1 - sigma, noise_b = sigma) - (1 - sigma) * scaling * shift (the shift is linear, so it
comes off afterwards; without noise the oracle applies no noise_a: - scaling * shift), packed with _pack_latents' view / permute / reshape.
fp16 tokens are held to the tolerance; the bf16 tokens of the same call are the same fp32 values rounded to 8 bits instead of 11, so they lie
within 2^-9 + 2^-12 < 2^-8 (relative) of the fp16 ones, element by element.

Sub-batches: a plan only splits a batch whose widest activation reaches 2^31 bytes (csrc/vae.cpp vae_plan_build) — nothing a shrunken shape
reaches, which is why tests/test_gpu_vae_multi.py goes to the true VAE at 1024^2 with batch 8 (two passes of 4).  The same here: the true Flux
VAE, batch 8, equals two batch-4 calls (one pass each, the same kernels on the same shapes) bit for bit, so the second pass wrote whole images
behind the first.
"""
import pytest
import torch

from oracle import vae_ref as VR

pytestmark = pytest.mark.gpu

SHIFT, SCALING, SIGMA = 0.1159, 0.3611, 0.35


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def pack(z):
    B, C, H, W = z.shape
    return z.view(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), C * 4)


@pytest.mark.parametrize("channels,img,batch", [((64, 128, 128), 64, 2), ((64, 128, 256, 256), 128, 3)])
def test_flux_vae_encode_packed_matches_oracle(channels, img, batch):
    from components.native import NativeVAEEncoder
    arch = dict(VR.tiny_arch(channels), latent_channels=16, use_quant_conv=False)
    P = VR.synth_params(arch, seed=0)
    assert "quant_conv.weight" not in P and P["encoder.conv_out.weight"].shape[0] == 32
    g = torch.Generator().manual_seed(1)
    image = (torch.rand(batch, 3, img, img, generator=g) * 2 - 1).half().float()
    lat = img >> (len(channels) - 1)
    eps = torch.randn(batch, 16, lat, lat, generator=g).half().float()
    noise = torch.randn(batch, 16, lat, lat, generator=g).half().float()
    enc = NativeVAEEncoder(dict(in_channels=3, latent_channels=16, block_out_channels=channels, layers_per_block=2, use_quant_conv=0),
                           device="cuda:0")
    enc.load_vae_state_dict({k: v.half() for k, v in P.items()})
    assert enc.ready()
    for e, n in ((eps, noise), (None, None)):                                    # sampled + noised; posterior mode
        ref = VR.prepare_latents(P, arch, image, e, n, SCALING, 1.0 - SIGMA, SIGMA)
        ref = pack(ref - ((1.0 - SIGMA) if n is not None else 1.0) * SCALING * SHIFT)
        got = enc.encode_packed(image, eps=e, noise=n, scaling_factor=SCALING, shift_factor=SHIFT, sigma=SIGMA, out_dtype=torch.float16).clone()
        gbf = enc.encode_packed(image, eps=e, noise=n, scaling_factor=SCALING, shift_factor=SHIFT, sigma=SIGMA, out_dtype=torch.bfloat16).clone()
        torch.cuda.synchronize()
        assert got.shape == ref.shape == (batch, lat * lat // 4, 64) and got.dtype == torch.float16 and gbf.dtype == torch.bfloat16
        err = rel_l2(got, ref)
        print("flux vae encode_packed %s img %d B %d %s: relative L2 %.2e" % (channels, img, batch, "sampled" if e is not None else "mode", err))
        assert err < 3e-3, err
        d = (gbf.float() - got.float()).abs()
        assert bool((d <= got.float().abs() * 2.0 ** -8 + 2.0 ** -24).all())
    assert len(enc._plans) == 1
    # the NCHW calls keep their limit of 8 latent channels: an error, not a wrong answer
    with pytest.raises(RuntimeError):
        enc.encode(image, eps=None, noise=None, scaling_factor=1.0)
        torch.cuda.synchronize()


def test_flux_vae_encode_packed_full_size_sub_batches():
    from components.native import VAE_CONFIGS, NativeVAEEncoder
    B, img = 8, 1024
    enc = NativeVAEEncoder(VAE_CONFIGS["flux"], device="cuda:0")
    enc.init_synthetic(3)
    assert enc.ready()
    g = torch.Generator().manual_seed(2)
    image = (torch.rand(B, 3, img, img, generator=g) * 2 - 1).half().cuda()
    eps = torch.randn(B, 16, 128, 128, generator=g).half().cuda()
    noise = torch.randn(B, 16, 128, 128, generator=g).half().cuda()
    kw = dict(scaling_factor=SCALING, shift_factor=SHIFT, sigma=SIGMA, out_dtype=torch.bfloat16)
    whole = enc.encode_packed(image, eps=eps, noise=noise, **kw).clone()
    halves = [enc.encode_packed(image[i:i + 4], eps=eps[i:i + 4], noise=noise[i:i + 4], **kw).clone() for i in (0, 4)]
    torch.cuda.synchronize()
    assert whole.shape == (B, 4096, 64) and torch.isfinite(whole.float()).all()
    assert torch.equal(whole[:4], halves[0]) and torch.equal(whole[4:], halves[1])
    assert not torch.equal(whole[:4], whole[4:])
