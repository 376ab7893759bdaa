"""The device image preprocessing without a GPU: the NumPy restatement of Pillow's 8-bit bicubic resize
(tests/pil_resample_oracle.py) against the installed Pillow, the C ABI's argument checks (which launch nothing), and the routing of
components/preproc.py and FeatureExtractor with stand-ins."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resample_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ("gdf_op_pil_coeffs", "gdf_op_pil_resize_workspace_bytes", "gdf_op_pil_resize_u8")


def _fake_diffusers():
    """tests/fake_diffusers' stub package under a private name (sys.modules['diffusers'] is left to the tests that install it)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_fake_diffusers_pil", os.path.join(ROOT, "tests", "fake_diffusers", "diffusers", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("hw,size", O.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_oracle_equals_pillow(hw, size):
    """every byte, for RGB noise, RGB of bytes 0 / 255 (both clamps) and L; if this fails on some Pillow build, the oracle is what to fix first"""
    for kind in O.KINDS:
        a = O.source(kind, *hw)
        want = np.array(Image.fromarray(a).resize((size, size)).convert("RGB"))
        got = O.resize_rgb(a, size)
        assert got.shape == want.shape == (size, size, 3) and np.array_equal(got, want), kind


def test_the_0_255_sources_reach_both_clamps():
    """bicubic overshoots between a 0 and a 255: the unclamped value of a pass leaves [0, 255] on both sides"""
    a = O.source("rgb01", 33, 47).astype(np.int64)
    bounds, kk, _ = O.coeffs(47, 128)
    v = np.stack([(1 << 21) + (a[:, lo:lo + n] * kk[xx, :n, None]).sum(1) >> 22 for xx, (lo, n) in enumerate(bounds)])
    assert v.min() < 0 and v.max() > 255


def test_oracle_tables_have_the_stated_shape():
    for n_in, n_out in O.axis_pairs():
        bounds, kk, ksize = O.coeffs(n_in, n_out)
        assert ksize == O.ksize_of(n_in, n_out) and kk.shape == (n_out, ksize)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert (np.abs(kk.sum(1) - (1 << 22)) <= ksize).all()                   # normalised to 1 in 2^22 fixed point, up to one rounding per tap
        for xx in range(n_out):
            assert not kk[xx, bounds[xx, 1]:].any()
    assert O.ksize_of(2048, 64) == 129 and O.ksize_of(1, 16) == 5


def test_normalisation_through_double_is_the_fp32_one():
    """the kernel divides in double and rounds to fp32 (csrc/preproc.hip pil_normalise): for all 256 bytes that is the correctly rounded fp32
    quotient, and the oracle's normalise is what both image processors make of the bytes"""
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal((u.astype(np.float64) / 255.0).astype(np.float32), u.astype(np.float32) / np.float32(255.0))
    a = O.source("rgb", 16, 16)
    from components.models import SyntheticPipe
    syn = SyntheticPipe._preprocess(None, Image.fromarray(a))
    assert torch.equal(syn[0], torch.from_numpy(O.normalise(a)))
    fake = _fake_diffusers().VaeImageProcessor(vae_scale_factor=8).preprocess(Image.fromarray(a))
    assert torch.equal(fake[0], torch.from_numpy(O.normalise(a)))


def test_symbols_are_exported_declared_and_bound():
    from components import native
    L = native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    for n in NEW_OPS:
        assert hasattr(L, n) and n in native.OP_SIGNATURES and getattr(L, n).argtypes == native.OP_SIGNATURES[n][1] and n + "(" in hdr, n
    import __graft_entry__ as G
    assert "preproc.hip" in G.SOURCES
    from components import preproc
    assert callable(preproc.device_preprocess)


def test_argument_checks_run_before_any_launch():
    """null pointers, channels, sizes, alignment: GDF_ERR_ARG; a source more than 32 times the target on an axis (ksize > 129) and 2^31 bytes:
    GDF_ERR_UNSUPPORTED; each with a message naming the entry, and nothing is launched (so this runs without a device)"""
    from components import native
    L = native.load_library()
    vp = C.c_void_p
    a = vp(4096)                                                               # never dereferenced: every call below is refused
    ks = C.c_int(-7)
    for bad in (dict(n_in=0), dict(n_out=0), dict(n_in=-3), dict(bounds=vp(0)), dict(kk=vp(0)), dict(ks=None), dict(bounds=vp(4098))):
        k = dict(dict(n_in=100, n_out=64, bounds=a, kk=a, ks=C.byref(ks)), **bad)
        assert L.gdf_op_pil_coeffs(k["n_in"], k["n_out"], k["bounds"], k["kk"], k["ks"], None) == 1, bad                # GDF_ERR_ARG
        assert b"gdf_op_pil_coeffs" in L.gdf_last_error(), bad
    assert L.gdf_op_pil_coeffs(2049, 64, a, a, C.byref(ks), None) == 4 and b"gdf_op_pil_coeffs" in L.gdf_last_error()      # GDF_ERR_UNSUPPORTED
    assert b"32" in L.gdf_last_error() and ks.value == -7

    for bad in (dict(src=vp(0)), dict(ws=vp(0)), dict(u8=vp(0), f32=vp(0)), dict(ch=2), dict(ch=4), dict(ch=0), dict(h=0), dict(w=0), dict(oh=0),
                dict(ow=-1), dict(f32=vp(4098)), dict(ws=vp(4104))):
        k = dict(dict(src=a, h=9, w=11, ch=3, oh=8, ow=8, u8=a, f32=a, ws=a), **bad)
        rc = L.gdf_op_pil_resize_u8(k["src"], k["h"], k["w"], k["ch"], k["oh"], k["ow"], k["u8"], k["f32"], k["ws"], None)
        assert rc == 1 and b"gdf_op_pil_resize_u8:" in L.gdf_last_error(), bad
    for h, w, oh, ow in ((8, 2049, 64, 64), (2049, 8, 64, 64), (33, 1, 1, 1)):
        assert L.gdf_op_pil_resize_u8(a, h, w, 3, oh, ow, a, a, a, None) == 4 and b"gdf_op_pil_resize_u8:" in L.gdf_last_error(), (h, w)
        assert L.gdf_op_pil_resize_workspace_bytes(h, w, 3, oh, ow) == 0
    assert L.gdf_op_pil_resize_u8(a, 32768, 32768, 3, 32768, 32768, a, a, a, None) == 4 and b"2^31" in L.gdf_last_error()
    assert L.gdf_op_pil_resize_workspace_bytes(9, 11, 2, 8, 8) == 0 and L.gdf_op_pil_resize_workspace_bytes(0, 11, 3, 8, 8) == 0

    def r16(v):
        return (v + 15) // 16 * 16
    # [horizontal bounds | kk | vertical bounds | kk | intermediate [src_h][out_w][C]] + 16; a skipped pass has no part
    both = r16(64 * 8) + r16(64 * O.ksize_of(70, 64) * 4) + r16(64 * 8) + r16(64 * O.ksize_of(90, 64) * 4) + r16(90 * 64 * 3) + 16
    assert L.gdf_op_pil_resize_workspace_bytes(90, 70, 3, 64, 64) == both
    assert L.gdf_op_pil_resize_workspace_bytes(100, 64, 1, 64, 64) == r16(64 * 8) + r16(64 * O.ksize_of(100, 64) * 4) + 16
    assert L.gdf_op_pil_resize_workspace_bytes(64, 64, 3, 64, 64) == 16
    assert L.gdf_op_pil_resize_workspace_bytes(2048, 2048, 3, 64, 64) > 0                                  # in / out = 32 exactly is taken


# ---- routing (components/preproc.py, FeatureExtractor), with stand-ins and no device ----
def _img(mode, w=20, h=14):
    g = np.random.default_rng(3)
    if mode == "I;16":
        return Image.fromarray(g.integers(0, 65536, (h, w), dtype=np.uint16))
    return Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).convert(mode)


def test_rgb_and_l_go_to_the_device_every_other_mode_to_the_host():
    from components import preproc as P
    assert P.route(_img("RGB"), 16) == "device" and P.route(_img("L"), 16) == "device"
    for mode in ("P", "1", "RGBA", "LA", "CMYK", "I;16", "F", "I"):
        assert P.route(_img(mode), 16) == "host", mode
    assert P.route(object(), 16) == "host"                                     # (not an image: the host function gets to say so)
    # a source more than 32 times the target on either axis is the C ABI's GDF_ERR_UNSUPPORTED: the host takes it
    assert P.route(_img("RGB", w=64, h=3), 2) == "device" and P.route(_img("RGB", w=65, h=3), 2) == "host" and P.route(_img("L", w=3, h=65), 2) == "host"


def test_mixed_batch_plan_packs_bytes_and_host_rows_at_16_byte_offsets():
    from components import preproc as P
    S = 8
    imgs = [_img("RGB", 21, 13), _img("RGBA"), _img("L", 7, 5), _img("P"), _img("RGB", S, S)]
    seen = []

    def host_fn(im):
        seen.append(im.mode)
        return P.default_host_fn(S)(im)
    items, total = P.plan_batch(imgs, S, host_fn)
    assert [k for k, _o, _a in items] == ["device", "host", "device", "host", "device"] and seen == ["RGBA", "P"]
    off = 0
    for (kind, o, a), im in zip(items, imgs):
        assert o == off and o % 16 == 0
        if kind == "device":
            assert a.dtype == np.uint8 and np.array_equal(a, np.asarray(im)) and a.flags.c_contiguous
        else:
            want = torch.from_numpy(O.normalise(np.array(im.resize((S, S)).convert("RGB"))))
            assert a.dtype == np.float32 and a.shape == (3, S, S) and torch.equal(torch.from_numpy(a), want)
        off += (a.nbytes + 15) // 16 * 16
    assert total == off


def test_flag_and_environment(monkeypatch):
    from components import preproc as P
    monkeypatch.delenv("GDF_DEVICE_PREPROCESS", raising=False)
    assert P.resolve_flag(None, "cuda:0") is False and P.resolve_flag(None, "cpu") is False                # the default is off
    assert P.resolve_flag(True, "cuda:0") is True and P.resolve_flag(True, "cuda") is True and P.resolve_flag(True, torch.device("cuda", 1)) is True
    assert P.resolve_flag(False, "cuda:0") is False and P.resolve_flag(False, "cpu") is False
    for v, on in (("1", True), ("true", True), ("on", True), ("0", False), ("", False), ("false", False), ("off", False)):
        monkeypatch.setenv("GDF_DEVICE_PREPROCESS", v)
        assert P.resolve_flag(None, "cuda:0") is on, v
        assert P.resolve_flag(None, "cpu") is False                                                  # a preference, not a demand
        assert P.resolve_flag(False, "cuda:0") is False and P.resolve_flag(True, "cuda:0") is True      # the keyword wins
    for dev in ("cpu", torch.device("cpu")):
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            P.resolve_flag(True, dev)
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            P.device_preprocess([_img("RGB")], 16, dev)


def test_extractor_routes_pil_batches_by_its_flag(monkeypatch):
    """FeatureExtractor._preprocess_images, the one place extract and _extract_multi make the batch of image_type='image'"""
    import diffusion_feature as D
    from components import preproc as P
    calls = []

    def fake(images, size, device, host_fn=None):
        calls.append((len(images), size, device, host_fn))
        return torch.full((len(images), 3, size, size), 7.0)
    monkeypatch.setattr(P, "device_preprocess", fake)
    fe = D.FeatureExtractor.__new__(D.FeatureExtractor)
    torch.nn.Module.__init__(fe)
    fe.img_size, fe.device = 16, "cuda:0"
    fe.pipe = types.SimpleNamespace(image_processor=types.SimpleNamespace(preprocess=P.default_host_fn(16)))
    imgs = [_img("RGB"), _img("L")]
    host = fe._preprocess_images(imgs)                                         # built without the keyword: the host path
    assert not calls and tuple(host.shape) == (2, 3, 16, 16) and torch.equal(host[1:], fe.preprocess_image(imgs[1]))
    fe.device_preprocess = True
    dev = fe._preprocess_images(imgs)
    assert len(calls) == 1 and calls[0][:3] == (2, 16, "cuda:0") and calls[0][3] == fe.preprocess_image and bool((dev == 7).all())
    assert torch.equal(fe.preprocess_images_device(imgs[:1]), dev[:1]) and len(calls) == 2
    src = open(D.__file__).read()
    assert src.count("self._preprocess_images(list(image))") == 2 and "_map_threads(self.preprocess_image" in src


def test_constructor_keyword_on_a_cpu_device_raises(monkeypatch):
    import diffusion_feature as D
    monkeypatch.setattr(D, "get_diffusion_model", lambda *a, **k: pytest.fail("the pipeline was built before the keyword was checked"))
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        D.FeatureExtractor(None, "1-5", "cpu", device_preprocess=True)
