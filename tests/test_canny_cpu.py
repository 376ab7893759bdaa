"""The device Canny without a GPU: the NumPy oracle (tests/canny_oracle.py) against the hand-checkable facts of DESIGN.md 3.19 and, where cv2 is
installed, against cv2.Canny; the byte round trip that lets the VAE's tensor stand in for the image bytes; exported / declared / bound symbols and
the argument checks that run before any launch; the routing of components/control.py and the CLI's input-path decision with stand-ins."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import canny_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ("gdf_op_canny_workspace_bytes", "gdf_op_canny_classify", "gdf_op_canny_link", "gdf_op_canny")


@pytest.mark.parametrize("name", list(O.steps()))
def test_oracle_reproduces_the_hand_checkable_facts(name):
    img, want = O.steps()[name]
    got = O.canny(img, 100, 200)
    assert set(np.unique(got)) <= {0, 255} and np.array_equal(got > 0, want), name
    cls = O.classify(img)
    if "green" in name:                                   # mag 4 * 40 = 160: in (100, 200]
        assert int((cls == O.CANDIDATE).sum()) == img.shape[0] and int((cls == O.STRONG).sum()) == 0
    else:
        assert int((cls == O.STRONG).sum()) == int(want.sum()) and int((cls == O.CANDIDATE).sum()) == 0
    assert np.array_equal(O.classify(img, 200, 100), cls)                                    # thresholds are swapped when low > high
    assert np.array_equal(O.classify(img, 100.9, 200.9), cls)                                # and floored


def test_oracle_border_rules_and_channel_choice():
    # replicated PIXEL border: a constant image has no gradient anywhere, also on its border
    assert not O.canny(np.full((9, 11, 3), 200, np.uint8)).any()
    # zero MAGNITUDE border: a gradient that is largest on the border column still survives the suppression there
    ramp = np.zeros((8, 8), np.uint8); ramp[:, 0] = 255
    assert (O.canny(ramp)[:, 0] == 255).all()
    # a one-channel image and its three-fold copy agree (ties go to the first channel, all three are equal)
    img = O.smooth_noise(1, 40, 56, C=0, seed=5)[0]
    assert np.array_equal(O.classify(img), O.classify(np.stack([img] * 3, axis=2)))
    # link: the flood and a dilation fixpoint agree on a random map
    cls = O.random_map(24, 40, 0.42, 0.01, seed=4)
    e = cls == O.STRONG
    while True:
        p = np.pad(e, 1)
        grown = np.zeros_like(e)
        for dy in range(3):
            for dx in range(3):
                grown |= p[dy:dy + 24, dx:dx + 40]
        nxt = e | (grown & (cls == O.CANDIDATE))
        if np.array_equal(nxt, e):
            break
        e = nxt
    assert np.array_equal(O.link(cls) > 0, e)


def test_crafted_link_maps_are_what_they_claim():
    """the crafted maps are what they claim: one component, its geodesic length of the order of its pixel count"""
    s = O.serpentine()
    assert int((s != O.NONE).sum()) == 7727 and int((s == O.STRONG).sum()) == 1
    assert int((O.link(s) > 0).sum()) == 7727 and not O.link(O.serpentine(strong=False)).any()
    d = O.diagonal()
    assert (O.link(d) > 0).sum() == (d != O.NONE).sum() and d[31, 31] == d[32, 32] == 0 and d[31, 96] == d[32, 95] == 0 and d[31, 32] == d[32, 31] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_byte_round_trip(dtype):
    """preprocess_image's 2 (u / 255) - 1, in fp32 and rounded to fp16, quantises back to u for all 256 bytes: the VAE's tensor gives the very
    bytes of _preprocess_basic(image)"""
    u = torch.arange(256, dtype=torch.uint8)
    t = (torch.from_numpy(np.asarray(u.numpy(), dtype=np.float32) / 255.0) * 2.0 - 1.0).to(dtype)          # components/models.py _preprocess
    assert torch.equal(O.quantise(t), u)
    t2 = (2.0 * (u.float() / 255.0) - 1.0).to(dtype)                                                       # diffusers' normalize
    assert torch.equal(O.quantise(t2), u)
    assert O.quantise(torch.tensor([-3.0, -1.0, 1.0, 7.0, float(np.float32(1 / 255) - 1)])).tolist() == [0, 0, 255, 255, 0]     # clamp; 0.5 -> even


def test_oracle_equals_cv2_where_installed():
    cv2 = pytest.importorskip("cv2")
    imgs = [O.smooth_noise(1, 96, 160, seed=3)[0], O.smooth_noise(1, 37, 53, seed=4)[0], O.smooth_noise(1, 130, 257, C=0, seed=5)[0],
            O.smooth_noise(1, 96, 160, sigma=3.0, contrast=0.35, seed=6)[0]] + [im for im, _ in O.steps().values()]
    for im in imgs:
        assert np.array_equal(cv2.Canny(im, 100, 200), O.canny(im, 100, 200)), im.shape
        assert np.array_equal(cv2.Canny(im, 200, 100), O.canny(im, 200, 100)), im.shape


def test_symbols_are_exported_declared_and_bound():
    from components import native
    L = native.load_library()
    hdr = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    for n in NEW_OPS:
        assert hasattr(L, n) and n in native.OP_SIGNATURES and getattr(L, n).argtypes == native.OP_SIGNATURES[n][1] and n + "(" in hdr, n
    assert callable(native.canny)
    import __graft_entry__ as G
    assert "canny.hip" in G.SOURCES


def test_argument_checks_run_before_any_launch():
    """sizes, the 32-bit label range, kinds, null and misaligned pointers: an error with a message naming the entry, and nothing is launched
    (so this runs without a device)"""
    from components import native
    L = native.load_library()
    vp = C.c_void_p
    assert L.gdf_op_canny_workspace_bytes(1, 1, 1) == 16 + 16 + 16
    n = 2 * 37 * 53
    assert L.gdf_op_canny_workspace_bytes(2, 37, 53) == (4 * n + 15) // 16 * 16 + 2 * ((n + 15) // 16 * 16)
    assert L.gdf_op_canny_workspace_bytes(0, 4, 4) == 0 and L.gdf_op_canny_workspace_bytes(2, 32768, 32768) == 0
    a = vp(4096)                                                                                          # never dereferenced: every call below is refused
    assert L.gdf_op_canny(a, 0, 2, 32768, 32768, 100, 200, a, 0, a, None) == 4 and b"2^31" in L.gdf_last_error()      # GDF_ERR_UNSUPPORTED
    assert L.gdf_op_canny_link(a, 1, 65536, 32768, a, 0, a, None) == 4 and b"gdf_op_canny_link" in L.gdf_last_error()
    assert L.gdf_op_canny_classify(a, 0, 1, 65536, 32768, 100, 200, a, None) == 4
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(src_kind=4), dict(src_kind=-1), dict(dst_kind=2), dict(src=vp(0)), dict(dst=vp(0)),
                dict(ws=vp(0)), dict(src=vp(4098)), dict(dst=vp(4100)), dict(ws=vp(4104))):
        k = dict(dict(src=a, src_kind=0, B=1, H=8, W=8, dst=a, dst_kind=0, ws=a), **bad)
        rc = L.gdf_op_canny(k["src"], k["src_kind"], k["B"], k["H"], k["W"], 100, 200, k["dst"], k["dst_kind"], k["ws"], None)
        assert rc == 1 and b"gdf_op_canny:" in L.gdf_last_error(), bad                                   # GDF_ERR_ARG
    assert L.gdf_op_canny_classify(a, 0, 1, 8, 8, 100, 200, vp(4100), None) == 1 and b"gdf_op_canny_classify" in L.gdf_last_error()
    assert L.gdf_op_canny_link(vp(0), 1, 8, 8, a, 0, a, None) == 1 and b"gdf_op_canny_link" in L.gdf_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.canny(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


# ---- routing (components/control.py), with stand-ins and no device ----
class _Stub:
    def __init__(self, block):
        self.block, self.calls = block, []

    def forward_raw(self, latents, t, ctx, text_embeds, time_ids, cond, shared_ctx=False, split=0, out=None):
        self.calls.append(cond)
        return self.block.clone()


def _pipe():
    return types.SimpleNamespace(vae_scale_factor=8, synthetic_weights=True, unet=types.SimpleNamespace(cfg={}))


def _run(cp, **kw):
    return cp.generate_control_info(kw.pop("images", None), torch.zeros(2, 4, 2, 3), torch.tensor([1.0]), torch.zeros(2, 7, 8), {}, **kw)


def test_hip_device_pipeline_routes_canny_to_the_device(monkeypatch):
    from PIL import Image
    from components import control as K
    from components import native
    seen = []

    def fake_canny(src, low, high, out="control"):
        seen.append((src, low, high, out))
        return (src[:, :1] > 0).half().expand(-1, 3, -1, -1)
    monkeypatch.setattr(native, "canny", fake_canny)
    monkeypatch.setitem(sys.modules, "cv2", None)                          # importing cv2 would raise
    monkeypatch.setitem(sys.modules, "controlnet_aux", None)
    g = torch.Generator().manual_seed(0)
    a, b = (torch.randn(64, generator=g).half() for _ in range(2))
    src = torch.randn(2, 3, 16, 24, generator=g)
    want = (src[:, :1] > 0).half().expand(-1, 3, -1, -1)
    for choices in (["canny"], ["canny-xl"]):
        sa = _Stub(a)
        cp = K.ControlNetPipeline(_pipe(), choices, "cuda:0", models=[sa])
        assert cp.needs_source() and not cp.needs_pil()
        seen.clear()
        out = _run(cp, source=src)
        assert len(seen) == 1 and seen[0][0] is src and seen[0][1:] == (100, 200, "control")
        assert torch.equal(sa.calls[0], want) and torch.equal(out, a)
    # two Canny ControlNets: ONE edge image, the fp16 sum of the blocks
    sa, sb = _Stub(a), _Stub(b)
    cp = K.ControlNetPipeline(_pipe(), ["canny", "canny"], "cuda:0", models=[sa, sb])
    seen.clear()
    out = _run(cp, source=src)
    assert len(seen) == 1 and sa.calls[0] is sb.calls[0] and torch.equal(out, a + b)
    # no source: named, not a silent fall-back to the host
    with pytest.raises(ValueError, match="control_image="):
        _run(cp)
    # control_image= wins: no preprocessor of any kind
    seen.clear()
    cimg = torch.rand(2, 3, 16, 24, generator=g)
    try:
        _run(cp, source=src, control_image=cimg)
    except Exception:                                                      # (without a device the hand-over to 'cuda:0' fails, after the routing)
        pass
    assert not seen
    cpu = K.ControlNetPipeline(_pipe(), ["canny"], "cpu", models=[_Stub(a)])
    _run(cpu, source=src, control_image=cimg)
    assert not seen and torch.equal(cpu.control[0].calls[0], cimg.half())
    # depth stays on the host, on a HIP device too
    dep = K.ControlNetPipeline(_pipe(), ["canny", "depth"], "cuda:0", models=[_Stub(a), _Stub(b)])
    assert dep.needs_pil() and dep.needs_source() and dep.device_route("canny") and not dep.device_route("depth")
    pil = [Image.fromarray(np.zeros((16, 24, 3), np.uint8))] * 2
    with pytest.raises(NotImplementedError, match="controlnet_aux.*control_image="):
        _run(dep, images=pil, source=src)
    assert K.device_preprocessed(["canny", "canny-xl"], "cuda:0") and not K.device_preprocessed(["canny", "depth"], "cuda:0")
    assert not K.device_preprocessed(["canny"], "cpu") and not K.device_preprocessed([], "cuda")


def test_other_devices_keep_the_host_route(monkeypatch):
    from PIL import Image
    from components import control as K
    from components import native
    monkeypatch.setattr(native, "canny", lambda *a, **k: pytest.fail("the device preprocessor on a non-HIP device"))
    seen = []

    def canny(img, lo, hi):
        seen.append((img.shape, lo, hi))
        return (img[:, :, 0] > 127).astype(np.uint8) * 255
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(Canny=canny))
    sa = _Stub(torch.zeros(4).half())
    cp = K.ControlNetPipeline(_pipe(), ["canny"], "cpu", models=[sa])
    assert cp.needs_pil() and not cp.needs_source()
    arr = np.random.default_rng(0).integers(0, 256, (2, 16, 24, 3), dtype=np.uint8)
    _run(cp, images=[Image.fromarray(x) for x in arr], source=torch.zeros(2, 3, 16, 24))
    assert seen == [((16, 24, 3), 100, 200)] * 2
    assert torch.equal(sa.calls[0][:, 0], torch.from_numpy(arr[..., 0] > 127).half())


def test_cli_keeps_the_loader_threads_for_device_preprocessors():
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    base = ["--version", "1-5", "--t", "50"]

    def parse(extra):
        try:
            return cli.parse_args(base + extra)
        except SystemExit:
            return cli.parse_args(base + ["--input_dir", "x", "--output_dir", "y"] + extra)
    dec = lambda extra, n=8, dev="cuda:0": cli.use_loader_threads(parse(extra), n, dev)
    assert dec([]) and dec(["--control", "canny"]) and dec(["--control", "canny-xl"]) and dec(["--control", "canny", "canny"])
    assert not dec(["--control", "depth"]) and not dec(["--control", "canny", "depth"])
    assert not dec(["--control", "canny"], n=0) and not dec([], n=0)
    assert not dec(["--control", "canny"], dev="cpu") and dec([], dev="cpu")
