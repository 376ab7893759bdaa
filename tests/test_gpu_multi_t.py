"""FeatureExtractor.extract(..., t=[t1, ..., tK]) and `extract_feature.py --t T1 T2 ...` (-m gpu, synthetic weights, 128 x 128 images — the
smallest size the extractor tests use): one VAE encode and one UNet forward of K * B rows for K timesteps of the same B images.

The equivalence checks carry NO tolerance.  The multi-timestep call draws eps = randn((K*B, L, h, w)), then noise = randn(...) — the draws of
the single-timestep call at batch K * B (components/models.py native_prepare_latents_multi) —, encodes the B images once and runs one UNet
forward of K * B rows.  The reference is assembled from TODAY's single-timestep pieces only, with the same plan batches and the same draws:
for every k, NativeVAEEncoder.encode (gdf_vae_encode, plan batch B) of the B images with slice k of those draws and the (a, b) that
scheduler_noise_scalars gives the single path; the K results stacked; then extract(t=t_k, image_type='latents') on those K * B rows — the
single path's own scheduler copy, scale_model_input, embeddings, UNet forward (plan batch K * B), hooks, feature_resize and attention
aggregation.  Rows k*B:(k+1)*B of every feature of that call equal the same rows of the multi-timestep call bit for bit.

Why the reference is not `extract(t=t_k)` on the B images tiled K times: that call runs the VAE encoder at plan batch K * B, the multi-timestep
call at plan batch B, and at 128 x 128 the encoder's bits depend on the plan batch — measured on an MI355X with the VAE of this test,
batch 6 against batch 2 on the same images and draws: 712 of 2048 latent elements differ by one fp16 ulp (posterior mode: 1341 of 2048), while
the three copies inside the batch-6 call agree bit for bit and the UNet gives identical bits for a uniform timestep and the per-row vector on
all 330 non-map hooks.  The cause is the GEMM dispatcher, not the new code: gemm_splitk_factor (csrc/gemm.hip) splits K when the 128-row
tiles of a launch fill less than the chip, which depends on M = batch * H * W, and a different K split is a different summation order.
Batch POSITION invariance, which the project states, holds; batch-SIZE invariance of the encoder does not at sizes this small (at 1024^2
every batch runs in sub-batches of the same 4 images).  gdf_vae_encode_multi against gdf_vae_encode on one plan: tests/test_gpu_vae_multi.py.
The tiled form itself runs where its premise holds: test_tiled_single_timestep_calls_without_split_k (a child process with GDF_SPLITK=0).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, TS, IMG = 2, [50, 400, 50], 128
K = len(TS)

LAYERS = {
    "1-5": {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True, "up-level2-repeat0-vit-block0-cross-map": True},
    "xl": {"up-level1-repeat1-vit-block0-out": True, "up-level2-repeat2-res-out": True, "up-level1-repeat0-vit-block0-cross-map": True},
}


def _images(seed=5):
    return torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _keep(f):
    return {k: v.clone() for k, v in f.items()}


def _single(df, prompt, img, t, n=None):
    torch.manual_seed(0)
    n = n or img.shape[0]
    return _keep(df.extract(prompt, batch_size=n, image=img, image_type="tensors", t=t))


def _multi(df, prompt, img, ts):
    torch.manual_seed(0)
    return _keep(df.extract(prompt, batch_size=img.shape[0], image=img, image_type="tensors", t=ts))


def _reference_latents(df, img, ts):
    """(K*B, 4, h, w) from today's single-timestep VAE call: the draws of the RNG contract, slice k encoded with timestep k's (a, b)"""
    import copy
    from components.models import scheduler_noise_scalars
    pipe = df.pipe
    n = len(ts) * B
    g = torch.Generator(device="cuda:0").manual_seed(1234)                 # SyntheticPipe.prepare_latents' default generator
    shape = (n, 4, IMG // 8, IMG // 8)
    eps = torch.randn(shape, generator=g, device="cuda:0", dtype=torch.float32)
    noise = torch.randn(shape, generator=g, device="cuda:0", dtype=torch.float32)
    out = []
    for k, t in enumerate(ts):
        pipe.scheduler = copy.deepcopy(df.scheduler_backup)                # as extract() picks its timestep
        pipe.scheduler.set_timesteps(1000, device="cpu")
        timesteps, _ = pipe.get_timesteps(1000, t / 1000, "cpu")
        a, b = scheduler_noise_scalars(pipe.scheduler, timesteps[:1].repeat(B))
        rows = slice(k * B, (k + 1) * B)
        out.append(pipe.native_vae.encode(img.cuda(), eps=eps[rows], noise=noise[rows], scaling_factor=float(pipe.vae.config.scaling_factor),
                                          noise_a=a, noise_b=b).to(torch.float16).clone())
    return torch.cat(out, 0)


def _check_against_singles(df, prompt, img, multi, keys):
    """rows k*B:(k+1)*B of the multi call == the same rows of today's extract(t=t_k) on the K*B reference latents (module docstring)"""
    lat = _reference_latents(df, img, TS)
    singles = {t: _keep(df.extract(prompt, batch_size=K * B, image=lat, image_type="latents", t=t)) for t in sorted(set(TS))}
    for t, s in singles.items():
        assert list(s.keys()) == keys                          # the same ids in the same (hook execution) order
    for k, t in enumerate(TS):
        rows = slice(k * B, (k + 1) * B)
        for hid in keys:
            a, b = multi[hid][rows], singles[t][hid][rows]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(a, b), "%s, timestep %d (rows %d:%d): %d of %d elements differ" % (
                hid, t, rows.start, rows.stop, int((a != b).sum()), a.numel())


@pytest.mark.parametrize("version", ["1-5", "xl"])
def test_multi_timestep_equals_single_timestep_calls(version, monkeypatch):
    """'1-5': PNDM family (identity scale_model_input); 'xl': Euler family with text_embeds / time_ids.  Hooks incl. a '*-map' one; on '1-5' also
    the aggregated attention=['up_cross'] feature."""
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    layer = dict(LAYERS[version])
    attention = ["up_cross"] if version == "1-5" else None
    df = diffusion_feature.FeatureExtractor(layer=layer, version=version, img_size=IMG, device="cuda:0", attention=attention)
    prompt = df.encode_prompt("a photo of a cat")
    img = _images()
    before = _single(df, prompt, img, 50)
    keys = list(before.keys())                                 # hook execution order, 'attn' last
    assert sorted(keys) == sorted(list(layer) + (["attn"] if attention else []))
    multi = _multi(df, prompt, img, TS)
    assert list(multi.keys()) == keys
    for hid in keys:
        assert multi[hid].shape[0] == K * B and tuple(multi[hid].shape[1:]) == tuple(before[hid].shape[1:])
        assert multi[hid].dtype == torch.float16 and torch.isfinite(multi[hid].float()).all()
    _check_against_singles(df, prompt, img, multi, keys)

    for hid in keys:
        g0, g1, g2 = (multi[hid][k * B:(k + 1) * B] for k in range(K))
        assert not torch.equal(g0, g2), hid                  # the two t = 50 groups: their own posterior sample and noise
        assert not torch.equal(g0, g1), hid                  # different timesteps

    # split_timesteps: K dicts of VIEWS of the stored tensors
    stored = df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=TS)
    parts = diffusion_feature.split_timesteps(stored, K)
    assert len(parts) == K
    for k, part in enumerate(parts):
        assert list(part.keys()) == keys
        for hid in keys:
            v = part[hid]
            assert v.shape[0] == B and v.untyped_storage().data_ptr() == stored[hid].untyped_storage().data_ptr()
            assert v.data_ptr() == stored[hid][k * B].data_ptr() and torch.equal(v, stored[hid][k * B:(k + 1) * B])
    del parts, stored, v

    # K = 1 through a list: the single-timestep call's bits (same draws at batch 1 * B)
    one = _multi(df, prompt, img, [50])
    for hid in keys:
        assert torch.equal(one[hid], before[hid]), hid
    # and the integer path is what it was before the multi-timestep calls
    after = _single(df, prompt, img, 50)
    for hid in keys:
        assert torch.equal(after[hid], before[hid]), hid


def test_multi_timestep_with_feature_resize(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    layer = {"up-level2-repeat2-res-out": True, "up-level2-repeat0-vit-block0-cross-map": True}
    df = diffusion_feature.FeatureExtractor(layer=layer, version="1-5", img_size=IMG, device="cuda:0", feature_resize=2)
    prompt = df.encode_prompt("a photo of a cat")
    img = _images(6)
    multi = _multi(df, prompt, img, TS)
    assert tuple(multi["up-level2-repeat2-res-out"].shape) == (K * B, 640, 4, 4)
    assert sorted(multi.keys()) == sorted(layer)
    _check_against_singles(df, prompt, img, multi, list(multi.keys()))


def test_multi_timestep_refusals(monkeypatch):
    """every unsupported combination raises before any work, and leaves the feature store empty"""
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    hook = "up-level2-repeat2-res-out"
    df = diffusion_feature.FeatureExtractor(layer={hook: True}, version="1-5", img_size=IMG, device="cuda:0")
    prompt = df.encode_prompt("a photo of a cat")
    img = _images()
    lat = torch.randn(B, 4, IMG // 8, IMG // 8).half()

    def refused(exc, image=img, image_type="tensors", t=(50, 400), patch=(), **kw):
        """patch: (object, attribute, value) triples in force for the refused call only"""
        assert len(df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=50)) == 1     # something is in the store
        with monkeypatch.context() as m:
            for obj, name, val in patch:
                m.setattr(obj, name, val)
            with pytest.raises(exc) as e:
                df.extract(prompt, batch_size=B, image=image, image_type=image_type, t=list(t), **kw)
            assert len(str(e.value)) > 20                               # a message that says why
            assert df.feature_store.stored_feats == {}

    refused(NotImplementedError, use_ddim_inversion=True)
    refused(NotImplementedError, use_control=True)
    refused(ValueError, image=lat, image_type="latents")
    refused(ValueError, t=())
    refused(ValueError, t=tuple(range(10, 100, 10)))                    # K = 9
    assert tuple(df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=[50, 400])[hook].shape) == (2 * B, 640, 8, 8)
    del df

    def refused_on(df2, prompt2, n_single):
        """a working extractor of another kind: its single-timestep call fills the store, t=[...] raises and leaves it empty"""
        assert len(df2.extract(prompt2, batch_size=B, image=img, image_type="tensors", t=50)) == n_single
        with pytest.raises(NotImplementedError) as e:
            df2.extract(prompt2, batch_size=B, image=img, image_type="tensors", t=[50, 400])
        assert len(str(e.value)) > 20 and df2.feature_store.stored_feats == {}

    # 'vae-out' requested through the layer set, as a user requests it
    dfv = diffusion_feature.FeatureExtractor(layer={hook: True, "vae-out": True}, version="1-5", img_size=IMG, device="cuda:0")
    refused_on(dfv, dfv.encode_prompt("a photo of a cat"), 2)
    del dfv
    # the PixArt and flux versions: extractors over tiny synthetic pipelines (those of test_gpu_pixart.py / test_gpu_flux.py)
    from components.models import SyntheticFluxPipe, SyntheticPixartPipe
    from oracle import flux_ref as FR, pixart_ref as PR
    dfp = diffusion_feature.FeatureExtractor(layer={"vit-block1-out": True}, version="pixart-sigma", img_size=IMG, device="cuda:0",
                                             external_model=SyntheticPixartPipe("pixart-sigma", "cuda:0", seed=0, cfg=PR.tiny_arch(heads=8, num_layers=2, sample_size=16), n_txt=20))
    refused_on(dfp, dfp.encode_prompt("a photo of a cat"), 1)
    del dfp
    from PIL import Image
    dff = diffusion_feature.FeatureExtractor(layer={"vit-block0-out": True}, version="flux", img_size=IMG, device="cuda:0",
                                             external_model=SyntheticFluxPipe("cuda:0", seed=0, cfg=FR.tiny_arch(num_layers=2, num_single_layers=2), n_txt=16))
    pil = [Image.fromarray((np.random.RandomState(0).rand(90, 70, 3) * 255).astype(np.uint8))] * B
    assert len(dff.extract("a photo of a cat", batch_size=B, image=pil, t=100)) == 1
    with pytest.raises(NotImplementedError):
        dff.extract("a photo of a cat", batch_size=B, image=pil, t=[100, 300])
    assert dff.feature_store.stored_feats == {}


# ---- a diffusers pipeline (tests/fake_diffusers: the branch a user with real checkpoints takes) ---------------------------------------------
def test_multi_timestep_on_a_diffusers_euler_pipeline(monkeypatch):
    """'2-1' through `diffusers` (tests/fake_diffusers): EulerDiscreteScheduler objects with diffusers' state — get_timesteps leaves begin_index
    on the scheduler, add_noise reads the sigma at it.  Distinct timesteps; the multi-timestep call's per-timestep noise scalars are those the
    single path's OWN prepare_latents hands to the encoder, its rows equal the single-timestep pieces bit for bit, and the refusal of a
    pipeline built with GDF_NATIVE_VAE=0."""
    fake = os.path.join(ROOT, "tests", "fake_diffusers")
    monkeypatch.syspath_prepend(fake)
    for v in ("GDF_SYNTHETIC_WEIGHTS", "GDF_VERIFY"):
        monkeypatch.delenv(v, raising=False)
    sys.modules.pop("diffusers", None)
    import diffusers
    diffusers.reset()
    try:
        import diffusion_feature
        ts, S = [50, 400, 800], 256
        layer = {"up-level1-repeat1-vit-block0-cross-q": True, "up-level2-repeat2-res-out": True}
        df = diffusion_feature.FeatureExtractor(layer=layer, version="2-1", device="cuda:0", img_size=S, verify=False)
        pipe = df.pipe
        assert isinstance(pipe.scheduler, diffusers.EulerDiscreteScheduler) and not getattr(pipe, "synthetic_weights", False)
        enc = pipe.native_vae
        seen = {"single": [], "multi": []}
        enc_encode, enc_multi = enc.encode, enc.encode_multi

        def rec_encode(image, **kw):
            seen["single"].append((float(kw["noise_a"]), float(kw["noise_b"])))
            return enc_encode(image, **kw)

        def rec_multi(image, **kw):
            seen["multi"].append(list(zip(map(float, kw["noise_a"]), map(float, kw["noise_b"]))))
            return enc_multi(image, **kw)
        monkeypatch.setattr(enc, "encode", rec_encode)
        monkeypatch.setattr(enc, "encode_multi", rec_multi)
        prompt = df.encode_prompt("a photo of a cat")
        img = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(8)) * 2 - 1
        torch.manual_seed(0)
        multi = _keep(df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=ts))
        assert len(seen["multi"]) == 1 and not seen["single"]
        # the single path's own prepare_latents, timestep by timestep: the scalars it gives the encoder
        for k, t in enumerate(ts):
            df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=t)
            assert seen["multi"][0][k] == seen["single"][-1], (t, seen["multi"][0][k], seen["single"][-1])
        sig = [b for _, b in seen["multi"][0]]
        assert sig[0] < sig[1] < sig[2] and all(a == 1.0 for a, _ in seen["multi"][0])              # Euler: x + sigma_t * noise
        # bits: the single-timestep pieces on the same draws (module docstring), the draws being the global CUDA generator's after manual_seed(0)
        torch.manual_seed(0)
        shape = (len(ts) * B, 4, S // 8, S // 8)
        eps = torch.randn(shape, device="cuda:0", dtype=torch.float32)
        noise = torch.randn(shape, device="cuda:0", dtype=torch.float32)
        lat = torch.cat([enc_encode(img.cuda(), eps=eps[k * B:(k + 1) * B], noise=noise[k * B:(k + 1) * B], scaling_factor=float(pipe.vae.config.scaling_factor),
                                    noise_a=a, noise_b=b).to(torch.float16).clone() for k, (a, b) in enumerate(seen["multi"][0])], 0)
        for k, t in enumerate(ts):
            single = df.extract(prompt, batch_size=len(ts) * B, image=lat, image_type="latents", t=t)
            rows = slice(k * B, (k + 1) * B)
            for hid in layer:
                assert torch.equal(multi[hid][rows], single[hid][rows]), (hid, t)
        del df, single, multi
        # GDF_NATIVE_VAE=0: the pipeline keeps diffusers' prepare_latents and has no native encoder to share between timesteps
        monkeypatch.setenv("GDF_NATIVE_VAE", "0")
        diffusers.reset()
        df = diffusion_feature.FeatureExtractor(layer=layer, version="1-5", device="cuda:0", img_size=S, verify=False)
        assert getattr(df.pipe, "native_vae", None) is None
        with pytest.raises(NotImplementedError, match="GDF_NATIVE_VAE"):
            df.extract(df.encode_prompt("x"), batch_size=B, image=img, image_type="tensors", t=[50, 400])
        assert df.feature_store.stored_feats == {}
    finally:
        diffusers.reset()
        sys.modules.pop("diffusers", None)
        torch.cuda.empty_cache()


def test_tiled_single_timestep_calls_without_split_k():
    """The check as first stated: rows k*B:(k+1)*B of extract(t=[...]) == the same rows of extract(t=t_k) — the single path's own
    prepare_latents — on the B images tiled K times.  It needs the VAE encoder to give the same bits at plan batch B and K*B, which at
    128 x 128 it does only when the GEMM dispatcher does not split K by M (module docstring); GDF_SPLITK=0 is read once per process, so the
    check runs in a child process (tests/multi_t_tiled_check.py) with that setting."""
    import subprocess
    env = dict(os.environ, GDF_SPLITK="0", GDF_SYNTHETIC_WEIGHTS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multi_t_tiled_check.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert "tiled check ok" in r.stdout


# ---- CLI --------------------------------------------------------------------------------------------------------------------------------
def _setup(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(0)
    (tmp_path / "imgs").mkdir()
    for n in ("a", "b", "c"):
        Image.fromarray((rs.rand(64, 64, 3) * 255).astype(np.uint8)).save(tmp_path / "imgs" / f"{n}.png")
    (tmp_path / "prompt.txt").write_text("a photo of a cat")
    layers = {"up-level1-repeat2-res-out": True, "up-level3-repeat0-vit-block0-self-k": True}
    (tmp_path / "layers.json").write_text(json.dumps(layers))
    return layers


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_several_timesteps(tmp_path, monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    import diffusion_feature
    from PIL import Image
    layers = _setup(tmp_path)
    base = ["--layer", str(tmp_path / "layers.json"), "--version", "1-5", "--img_size", "128", "-b", "2", "--seed", "0",
            "--input_dir", str(tmp_path / "imgs" / "*.png"), "--prompt_file", str(tmp_path / "prompt.txt"), "--use_original_filename"]
    cli.main(base + ["--t", "100", "--output_dir", str(tmp_path / "one")])
    single_tree = _tree(tmp_path / "one")
    assert single_tree == sorted(os.path.join(k, f"{n}.npy") for k in layers for n in "abc")          # the layout without t<T>/ directories

    cli.main(base + ["--t", "100", "300", "--output_dir", str(tmp_path / "two")])
    assert sorted(os.listdir(tmp_path / "two")) == ["t100", "t300"]
    for t in ("t100", "t300"):
        assert _tree(tmp_path / "two" / t) == single_tree
    for k, (c, hw) in {"up-level1-repeat2-res-out": (1280, 4), "up-level3-repeat0-vit-block0-self-k": (320, 16)}.items():
        for n in "abc":
            x, y = np.load(tmp_path / "two" / "t100" / k / f"{n}.npy"), np.load(tmp_path / "two" / "t300" / k / f"{n}.npy")
            assert x.shape == y.shape == (c, hw, hw) and x.dtype == np.float16 and np.isfinite(x.astype(np.float32)).all()
            assert not np.array_equal(x, y)

    with pytest.raises(SystemExit) as e:                                   # their directories would collide
        cli.main(base + ["--t", "100", "100", "--output_dir", str(tmp_path / "dup")])
    assert e.value.code not in (0, None)
    assert not os.path.exists(tmp_path / "dup")

    # the single --t run wrote the bits of the single-timestep API call on the same batches
    df = diffusion_feature.FeatureExtractor(str(tmp_path / "layers.json"), "1-5", device="cuda", img_size=128)
    prompt = df.encode_prompt("a photo of a cat")
    for i, names in ((0, "ab"), (2, "c")):
        torch.manual_seed(0 + i)
        feats = df.extract(prompt, len(names), [Image.open(tmp_path / "imgs" / f"{n}.png") for n in names], t=100)
        for k in layers:
            for j, n in enumerate(names):
                got = np.load(tmp_path / "one" / k / f"{n}.npy")
                assert np.array_equal(got.view(np.uint16), feats[k][j].cpu().numpy().view(np.uint16)), (k, n)
