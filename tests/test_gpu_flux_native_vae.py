"""GDF_FLUX_NATIVE_VAE=1 (-m gpu): the Flux pipelines prepare their latents through the native 16-channel VAE (components/models.py
native_flux_prepare_latents, NativeVAEEncoder.encode_packed).

 * the real-checkpoint branch on the stub diffusers (set up like test_gpu_diffusers_branch.py::test_flux_real_checkpoint_branch_stock_pipeline):
   pipe.prepare_latents is the native drop-in, and what the transformer received as hidden_states is, bit for bit, encode_packed called
   directly on the preprocessed images with the same eps / noise (re-drawn from an equal generator state), the sigma of the scheduler's
   t_start and the VAE config's shift and scaling; img_ids are the pipeline's own.  (The arithmetic is covered at small sizes by
   test_gpu_vae_packed.py and test_gpu_vae_flux_encode.py; a full-size CPU oracle run is too slow for a test.)
 * without the variable pipe.prepare_latents stays the pipeline's own method;
 * SyntheticFluxPipe (shrunken transformer, as tests/test_gpu_flux.py builds it): last_call['hidden_states'] is encode_packed's output and
   the hooks are finite.
"""
import numpy as np
import pytest
import torch

from test_gpu_diffusers_branch import D, _images  # noqa: F401  (D: the fixture that puts tests/fake_diffusers on the path)

pytestmark = pytest.mark.gpu

LAYER = {"vit-block0-q": True, "vit-block1-out": True}


def test_stub_pipeline_prepares_latents_natively(D, monkeypatch):
    import diffusion_feature
    from components import models as M
    from components.native import NativeVAEEncoder
    monkeypatch.setenv("FAKE_DIFFUSERS_FLUX_LAYERS", "1,1")
    monkeypatch.setenv("GDF_FLUX_NATIVE_VAE", "1")
    df = diffusion_feature.FeatureExtractor(layer=LAYER, version="flux", device="cuda:0", img_size=1024)
    pipe, tr = df.pipe, df.pipe.transformer
    assert isinstance(pipe.native_vae, NativeVAEEncoder) and pipe.native_vae.ready()
    assert pipe.native_vae.cfg["latent_channels"] == 16 and pipe.native_vae.cfg["use_quant_conv"] == 0
    assert pipe.prepare_latents.__func__ is M.native_flux_prepare_latents
    native = pipe.prepare_latents
    rec = {}

    def recording(image, timestep, *a, **k):                       # the arguments and the generator state the call starts from
        rec.update(image=image.detach().clone(), timestep=timestep.clone(), args=a, state=torch.cuda.get_rng_state(torch.device("cuda:0")))
        return native(image, timestep, *a, **k)
    pipe.prepare_latents = recording
    vc = pipe.vae.config
    assert (vc.shift_factor, vc.scaling_factor) == (0.1159, 0.3611)
    dev = torch.device("cuda:0")
    # the first call of a real checkpoint still has the transformer's range check armed: the operand type is not settled and the latents travel
    # in the pipeline's bf16; from the second call on they are written in the operand type of the 'auto' mode, fp16
    for call, want_dtype in enumerate((torch.bfloat16, torch.float16)):
        assert (tr._range_check_sd is not None) == (call == 0)
        torch.manual_seed(11 + call)
        feats = df.extract("a macro photo of a dragonfly", batch_size=2, image=_images(2, 640, seed=7 + call), t=300)
        torch.cuda.synchronize()
        assert pipe.transformer_calls == call + 1 and tr.calls == call + 1 and tr.io_dtype == torch.float16
        kw = pipe.last_transformer_kwargs
        hs = kw["hidden_states"].clone()
        assert hs.shape == (2, 4096, 64) and hs.dtype == want_dtype
        assert all(torch.isfinite(v.float()).all() for v in feats.values()) and list(feats) == list(LAYER)
        # strength 0.3 of 28 steps: t_start = 19 (test_flux_real_checkpoint_branch_stock_pipeline); the scheduler's own table entry
        assert pipe.scheduler._begin_index == 19
        sigma = float(pipe.scheduler.sigmas[19])
        assert abs(sigma - kw["sigma"]) < 1e-3
        assert M.flux_scale_noise_sigma(pipe.scheduler, rec["timestep"]) == sigma
        after = torch.cuda.get_rng_state(dev)
        torch.cuda.set_rng_state(rec["state"], dev)
        eps = torch.randn((2, 16, 128, 128), device=dev, dtype=torch.float32)
        noise = torch.randn((2, 16, 128, 128), device=dev, dtype=torch.float32)
        torch.cuda.set_rng_state(after, dev)
        assert rec["image"].shape == (2, 3, 1024, 1024)
        want = pipe.native_vae.encode_packed(rec["image"], eps=eps, noise=noise, scaling_factor=vc.scaling_factor, shift_factor=vc.shift_factor,
                                             sigma=sigma, out_dtype=want_dtype)
        torch.cuda.synchronize()
        assert torch.equal(hs, want), call
        assert float(hs.float().std()) > 0.05 and not torch.equal(hs[0], hs[1])
        ids = D.FluxImg2ImgPipeline._prepare_latent_image_ids(2, 64, 64, dev, rec["args"][4])
        assert rec["args"][4] == torch.bfloat16 and kw["img_ids"].dtype == ids.dtype and torch.equal(kw["img_ids"], ids)
    with pytest.raises(NotImplementedError):
        native(rec["image"], rec["timestep"], 2, 16, 1024, 1024, torch.bfloat16, torch.device("cuda:0"), None, latents=hs)


def test_switch_off_keeps_the_pipelines_own_prepare_latents(D, monkeypatch):
    import diffusion_feature
    monkeypatch.setenv("FAKE_DIFFUSERS_FLUX_LAYERS", "1,1")
    monkeypatch.delenv("GDF_FLUX_NATIVE_VAE", raising=False)
    df = diffusion_feature.FeatureExtractor(layer=LAYER, version="flux", device="cuda:0", img_size=1024)
    assert df.pipe.prepare_latents.__func__ is D.FluxImg2ImgPipeline.prepare_latents
    assert getattr(df.pipe, "native_vae", None) is None


def test_synthetic_flux_pipe_uses_the_native_vae(monkeypatch):
    from PIL import Image
    import diffusion_feature
    from components.models import SyntheticFluxPipe
    from components.native import NativeVAEEncoder
    from oracle import flux_ref as FR
    monkeypatch.setenv("GDF_FLUX_NATIVE_VAE", "1")
    arch = FR.tiny_arch(num_layers=1, num_single_layers=1)
    pipe = SyntheticFluxPipe("cuda:0", seed=0, cfg=arch, n_txt=16)
    assert isinstance(pipe.native_vae, NativeVAEEncoder) and pipe.native_vae.ready()
    df = diffusion_feature.FeatureExtractor(layer={"vit-block0-out": True, "vit-block1-out": True}, version="flux", img_size=128, device="cuda:0",
                                            external_model=pipe)
    imgs = [Image.fromarray((np.random.RandomState(s).rand(90, 70, 3) * 255).astype(np.uint8)) for s in (0, 1)]
    feats = df.extract("a photo of a cat", batch_size=2, image=imgs, t=300)
    torch.cuda.synchronize()
    lc = pipe.last_call
    hs = lc["hidden_states"].clone()
    assert hs.shape == (2, 64, 64) and hs.dtype == pipe.transformer.io_dtype
    assert len(feats) == 2 and all(torch.isfinite(v.float()).all() for v in feats.values())
    x = torch.cat([pipe.image_processor.preprocess(i.resize((128, 128)).convert("RGB")) for i in imgs], 0).to("cuda:0", torch.float32)
    g = torch.Generator(device="cuda:0").manual_seed(1234)
    eps = torch.randn((2, 16, 16, 16), generator=g, device="cuda:0")
    noise = torch.randn((2, 16, 16, 16), generator=g, device="cuda:0")
    want = pipe.native_vae.encode_packed(x, eps=eps, noise=noise, scaling_factor=0.3611, shift_factor=0.1159, sigma=lc["sigma"],
                                         out_dtype=pipe.transformer.io_dtype)
    torch.cuda.synchronize()
    assert torch.equal(hs, want) and float(hs.float().std()) > 0.05


def test_synthetic_flux_pipe_switch_off_has_no_native_vae(monkeypatch):
    from components.models import SyntheticFluxPipe
    from oracle import flux_ref as FR
    monkeypatch.delenv("GDF_FLUX_NATIVE_VAE", raising=False)
    pipe = SyntheticFluxPipe("cuda:0", seed=0, cfg=FR.tiny_arch(num_layers=1, num_single_layers=1), n_txt=16)
    assert pipe.native_vae is None
