"""FeatureExtractor(device_preprocess=True) end to end (-m gpu): every hook of extract() equals, bit for bit, that of an extractor that
preprocesses on the host, over a mixed batch — RGB sources of two sizes, one L, one RGBA and one P (the last two fall back to the host image by
image).  '1-5' with synthetic weights at 128 x 128 as in tests/test_gpu_canny_extract.py (plain, t=[...], use_control with the device Canny), and
the tiny PixArt pipeline of tests/test_gpu_pixart.py."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import pixart_ref as PR

pytestmark = pytest.mark.gpu
LAYERS = ["down-level1-repeat1-vit-out", "mid-repeat1-res-out", "up-level1-repeat1-vit-block0-cross-q", "up-level3-repeat2-res-out"]
DIT_LAYERS = ["vit-block0-cross-q", "vit-block1-ffn-inner", "vit-block1-out"]
S = 128


def _smooth(g, h, w, c=3):
    """a low-frequency image with some noise on it (edges for Canny, and not a constant anywhere)"""
    y, x = np.mgrid[0:h, 0:w]
    ch = [127 + 90 * np.sin(x / (5.0 + 3 * k) + g.uniform(0, 6)) * np.cos(y / (7.0 + 2 * k) + g.uniform(0, 6)) + g.normal(0, 6, (h, w)) for k in range(c)]
    a = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return a if c == 3 else a[..., 0]


def _batch(seed):
    g = np.random.default_rng(seed)
    a, b = Image.fromarray(_smooth(g, 150, 130)), Image.fromarray(_smooth(g, 97, 211))
    return [a, b, Image.fromarray(_smooth(g, 140, 100, c=1)), Image.fromarray(_smooth(g, S, S)).convert("RGBA"), b.convert("P")]


@pytest.fixture(scope="module")
def unet_pair():
    """(host-path extractor, device-path extractor, prompt): '1-5', synthetic weights (seeded: the same in both), one Canny ControlNet"""
    mp = pytest.MonkeyPatch()
    mp.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    mp.delenv("GDF_DEVICE_PREPROCESS", raising=False)
    try:
        import diffusion_feature
        kw = dict(layer={k: True for k in LAYERS}, version="1-5", img_size=S, device="cuda:0", control=["canny"])
        host = diffusion_feature.FeatureExtractor(**kw)
        dev = diffusion_feature.FeatureExtractor(device_preprocess=True, **kw)
        assert host.device_preprocess is False and dev.device_preprocess is True
        yield host, dev, host.encode_prompt("a photo of a cat")
    finally:
        mp.undo()


def _keep(f):
    return {k: v.clone() for k, v in f.items()}


def _same(a, b, layers=LAYERS):
    assert list(a) == list(b) == layers
    for k in layers:
        assert a[k].dtype == torch.float16 and bool(torch.isfinite(a[k].float()).all()) and torch.equal(a[k], b[k]), k


def test_the_batch_itself(unet_pair):
    host, dev, _ = unet_pair
    pil = _batch(1)
    assert [i.mode for i in pil] == ["RGB", "RGB", "L", "RGBA", "P"]
    got = dev.preprocess_images_device(pil)
    want = torch.concat([host.preprocess_image(i) for i in pil], dim=0)
    assert got.is_cuda and tuple(got.shape) == (5, 3, S, S) and torch.equal(got.cpu(), want)


def test_plain_extraction(unet_pair, monkeypatch):
    host, dev, prompt = unet_pair
    pil = _batch(2)
    from components import preproc
    calls, real = [], preproc.device_preprocess

    def counting(images, *a, **k):
        calls.append(len(images))
        return real(images, *a, **k)
    monkeypatch.setattr(preproc, "device_preprocess", counting)
    got = _keep(dev.extract(prompt, batch_size=5, image=pil, t=50))
    assert calls == [5]                                                       # the device path made this batch ...
    want = _keep(host.extract(prompt, batch_size=5, image=pil, t=50))
    assert calls == [5]                                                       # ... and the host path the other
    _same(got, want)


def test_two_timesteps(unet_pair):
    host, dev, prompt = unet_pair
    pil = _batch(3)
    got = _keep(dev.extract(prompt, batch_size=5, image=pil, t=[50, 400]))
    want = _keep(host.extract(prompt, batch_size=5, image=pil, t=[50, 400]))
    assert got[LAYERS[0]].shape[0] == 10
    _same(got, want)


def test_use_control_with_the_device_canny(unet_pair):
    host, dev, prompt = unet_pair
    pil = _batch(4)
    got = _keep(dev.extract(prompt, batch_size=5, image=pil, t=50, use_control=True))
    want = _keep(host.extract(prompt, batch_size=5, image=pil, t=50, use_control=True))
    _same(got, want)
    plain = _keep(dev.extract(prompt, batch_size=5, image=pil, t=50))
    assert not torch.equal(got[LAYERS[-1]], plain[LAYERS[-1]])                # the ControlNet acted


def test_back_to_back_calls_without_a_synchronise(unet_pair):
    """two extract calls on different images, the second queued while the first may still be running: the staging buffer of the first is
    not rewritten under its copy"""
    host, dev, prompt = unet_pair
    p1, p2 = _batch(5), _batch(6)[::-1]
    torch.cuda.synchronize()
    a = _keep(dev.extract(prompt, batch_size=5, image=p1, t=50))
    b = _keep(dev.extract(prompt, batch_size=5, image=p2, t=50))
    want_a = _keep(host.extract(prompt, batch_size=5, image=p1, t=50))
    want_b = _keep(host.extract(prompt, batch_size=5, image=p2, t=50))
    _same(a, want_a)
    _same(b, want_b)
    assert not torch.equal(a[LAYERS[0]], b[LAYERS[0]])


def test_pixart(monkeypatch):
    monkeypatch.delenv("GDF_DEVICE_PREPROCESS", raising=False)
    import diffusion_feature
    from components.models import SyntheticPixartPipe
    arch = PR.tiny_arch(heads=8, num_layers=2, sample_size=16)
    layer = {k: True for k in DIT_LAYERS}
    out = []
    pil = _batch(7)
    for flag in (None, True):
        pipe = SyntheticPixartPipe("pixart-sigma", "cuda:0", seed=0, cfg=arch, n_txt=20)
        df = diffusion_feature.FeatureExtractor(layer=layer, version="pixart-sigma", img_size=S, device="cuda:0", external_model=pipe,
                                                device_preprocess=flag)
        assert df.device_preprocess is bool(flag)
        out.append(_keep(df.extract(df.encode_prompt("a photo of a cat"), batch_size=5, image=pil, t=100)))
    _same(out[1], out[0], DIT_LAYERS)
