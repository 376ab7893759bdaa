"""The reference's own use_control call forms on the native path (-m gpu): FeatureExtractor(control=['canny']).extract(use_control=True) from PIL
images and from tensors, with the Canny preprocessor a device kernel (csrc/canny.hip) — no cv2 anywhere: importing it raises in every test here.
Synthetic weights, version 1-5 at 128 x 128 as in tests/test_gpu_controlnet_model.py.  Hooks are compared bit for bit with the same call given the
edge images ready-made (control_image=), those built by the NumPy oracle (tests/canny_oracle.py) from _preprocess_basic of the same images."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import canny_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ["down-level1-repeat1-vit-out", "mid-repeat1-res-out", "up-level1-repeat1-vit-block0-cross-q", "up-level3-repeat2-res-out"]
S = 128


@pytest.fixture(autouse=True)
def _no_cv2(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")


@pytest.fixture(scope="module")
def fx():
    """one extractor with one Canny ControlNet and its prompt, shared by the tests below (none of them changes it)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    try:
        import diffusion_feature
        df = diffusion_feature.FeatureExtractor(layer={k: True for k in LAYERS}, version="1-5", img_size=S, device="cuda:0", control=["canny"])
        yield df, df.encode_prompt("a photo of a cat")
    finally:
        mp.undo()


def _pil(n=2, size=(150, 130)):
    from PIL import Image
    return [Image.fromarray(im) for im in O.smooth_noise(n, size[1], size[0], seed=21)]


def _edges(df, pil):
    """(B, 3, S, S) fp32 of 0 / 1: the reference's three-channel edge image / 255, by the oracle, from _preprocess_basic of the images"""
    e = np.stack([O.canny(np.array(df._preprocess_basic(im)), 100, 200) for im in pil])
    assert e.any() and not e.all()
    return torch.from_numpy(e > 0).float()[:, None].expand(-1, 3, -1, -1).contiguous()


def _keep(f):
    return {k: v.clone() for k, v in f.items()}


def _same(a, b):
    assert list(a) == list(b) == LAYERS
    for k in LAYERS:
        assert a[k].dtype == torch.float16 and torch.equal(a[k], b[k]), k


def test_use_control_from_pil_images(fx):
    df, prompt = fx
    pil = _pil()
    got = _keep(df.extract(prompt, batch_size=2, image=pil, t=50, use_control=True))
    want = _keep(df.extract(prompt, batch_size=2, image=pil, t=50, use_control=True, control_image=_edges(df, pil)))
    _same(got, want)
    plain = _keep(df.extract(prompt, batch_size=2, image=pil, t=50))
    for k in LAYERS:                                                              # the ControlNet acts, and on the up path only
        assert bool(torch.isfinite(got[k].float()).all()) and torch.equal(got[k], plain[k]) == (not k.startswith("up-")), k


def test_use_control_from_tensors_at_img_size(fx):
    df, prompt = fx
    pil = _pil()
    x = torch.cat([df.preprocess_image(im) for im in pil], 0)
    assert tuple(x.shape) == (2, 3, S, S)
    from_pil = _keep(df.extract(prompt, batch_size=2, image=pil, t=50, use_control=True))
    _same(_keep(df.extract(prompt, batch_size=2, image=x, image_type="tensors", t=50, use_control=True)), from_pil)
    # the CLI's loader threads hand over fp16: the same bytes for Canny (whether the VAE sees the same latents is tests/test_gpu_cli.py's business)
    x16 = x.half()
    a = _keep(df.extract(prompt, batch_size=2, image=x16, image_type="tensors", t=50, use_control=True))
    b = _keep(df.extract(prompt, batch_size=2, image=x16, image_type="tensors", t=50, use_control=True, control_image=_edges(df, pil)))
    _same(a, b)


def test_use_control_from_a_tensor_of_another_size(fx):
    """the reference, literally: restore the tensor to PIL images, _preprocess_basic (PIL's resize), Canny of those bytes"""
    df, prompt = fx
    g = torch.Generator().manual_seed(5)
    small = torch.from_numpy(O.smooth_noise(2, 96, 112, seed=33)).permute(0, 3, 1, 2).float() / 255 * 2 - 1
    small = (small + 0.002 * torch.randn(small.shape, generator=g)).clamp(-1, 1)
    pil = df.restore_from_tensor_to_image(small)
    assert pil[0].size == (112, 96) and np.array_equal(np.array(pil[1]), O.quantise(small[1]).permute(1, 2, 0).numpy())
    got = _keep(df.extract(prompt, batch_size=2, image=small, image_type="tensors", t=50, use_control=True))
    want = _keep(df.extract(prompt, batch_size=2, image=small, image_type="tensors", t=50, use_control=True, control_image=_edges(df, pil)))
    _same(got, want)


def test_two_canny_controlnets_share_one_edge_image():
    import diffusion_feature
    from components import native
    df = diffusion_feature.FeatureExtractor(layer={k: True for k in LAYERS}, version="1-5", img_size=S, device="cuda:0", control=["canny", "canny"])
    cp = df.control_pipe
    assert len(cp.control) == 2 and cp.needs_source() and not cp.needs_pil()
    prompt = df.encode_prompt("a photo of a cat")
    pil = _pil()
    got = _keep(df.extract(prompt, batch_size=2, image=pil, t=50, use_control=True))
    want = _keep(df.extract(prompt, batch_size=2, image=pil, t=50, use_control=True, control_image=_edges(df, pil)))
    _same(got, want)
    # the block is the fp16 sum of the two models' blocks on ONE edge image
    calls = []
    real = native.canny

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 4, S // 8, S // 8, generator=g).half().cuda()
    ctx = prompt[0].repeat(2, 1, 1).cuda()
    tt = torch.tensor([500.0])
    src = torch.cat([df.preprocess_image(im) for im in pil], 0).cuda()
    native.canny = counting
    try:
        block = cp.generate_control_info(None, lat, tt, ctx, {}, source=src, shared_ctx=True, split=0).clone()
    finally:
        native.canny = real
    cond = _edges(df, pil).half().cuda()
    b0, b1 = (m.forward_raw(lat, tt, ctx, None, None, cond, shared_ctx=True, split=0).clone() for m in cp.control)
    torch.cuda.synchronize()
    assert len(calls) == 1 and block.dtype == torch.float16 and not torch.equal(b0, b1) and torch.equal(block, b0 + b1)


def test_cli_control_canny_keeps_the_loader_threads(tmp_path):
    """--control canny with loader threads writes files byte-identical to --loader_threads 0; neither path touches cv2"""
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    from PIL import Image
    (tmp_path / "imgs").mkdir()
    for n, im in zip("abc", O.smooth_noise(3, 100, 120, seed=44)):
        Image.fromarray(im).save(tmp_path / "imgs" / f"{n}.png")
    (tmp_path / "prompt.txt").write_text("a photo of a cat")
    layers = ["up-level1-repeat2-res-out", "up-level3-repeat0-vit-block0-self-k"]
    (tmp_path / "layers.json").write_text(json.dumps({k: True for k in layers}))
    base = ["--layer", str(tmp_path / "layers.json"), "--version", "1-5", "--img_size", str(S), "--t", "100", "-b", "2", "--control", "canny",
            "--input_dir", str(tmp_path / "imgs" / "*.png"), "--prompt_file", str(tmp_path / "prompt.txt")]
    seen = []
    real = cli.BatchLoader

    class Spy(real):
        def __init__(self, *a, **k):
            seen.append(1)
            super().__init__(*a, **k)
    cli.BatchLoader = Spy
    try:
        cli.main(base + ["--output_dir", str(tmp_path / "serial"), "--loader_threads", "0"])
        assert not seen
        cli.main(base + ["--output_dir", str(tmp_path / "threads"), "--loader_threads", "2"])
        assert seen == [1]                                                        # the loader-thread path really ran
    finally:
        cli.BatchLoader = real
    for k in layers:
        for i in range(3):
            a = np.load(tmp_path / "serial" / k / f"train{i}.npy")
            b = np.load(tmp_path / "threads" / k / f"train{i}.npy")
            assert a.dtype == b.dtype == np.float16 and np.array_equal(a.view(np.uint16), b.view(np.uint16)), (k, i)
