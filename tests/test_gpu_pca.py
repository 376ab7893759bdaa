"""The PCA of feature maps on the GPU (-m gpu): the kernels of csrc/pca.hip through gdf_op_pca / gdf_op_pca_rgb (include/gdf_ops.h),
components/postproc.py pca / pca_rgb and FeatureExtractor.visualize.

Kernel level: ONE run per case against the float64 oracle of tests/pca_ref.py with the bounds that file derives from the fp32 restatement's own error
on the same input (MARGIN x; no measured figure).  Every output is guard-filled and the workspace guard-tailed as in tests/test_gpu_clip_loss.py:
the owned elements written, everything behind them and behind the reported workspace size untouched."""
import ctypes
import gc
import warnings

import numpy as np
import pytest
import torch

import pca_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import bits, guard, is_guard

pytestmark = pytest.mark.gpu
PAT8, TAIL, PAD = 0xA5, 4096, 64


def _lib():
    return R.bind(lib())


def on_device(x, layout):
    """numpy (B, C, H, W) -> a device tensor of that logical shape: NCHW contiguous, channels-last, or an offset view into a NaN-filled
    channels-last buffer whose pixels are 8 channels longer than C"""
    t = torch.from_numpy(x).cuda()
    if layout == "nchw":
        return t
    if layout == "cl":
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert layout == "view"
    B, C_, H, W = t.shape
    buf = torch.full((B, H + 1, W + 2, C_ + 8), float("nan"), dtype=t.dtype, device="cuda")
    v = buf[:, :H, 1:W + 1, :C_].permute(0, 3, 1, 2)
    v.copy_(t)
    assert not v.is_contiguous() and v.stride(3) == C_ + 8
    return v


class Run:
    """one gdf_op_pca (and gdf_op_pca_rgb) on a device tensor, guard checks included; results as numpy arrays"""

    def __init__(self, d, k=3, joint=False, max_iter=R.MAX_ITER, tol=R.TOL, st=None, projection=True, size=None):
        L = _lib()
        B, C_, H, W = d.shape
        G = 1 if joint else B
        st = st if st is not None else stream()
        sizes = dict(mean=G * C_, components=G * k * C_, variance=G * k, total_variance=G, projection=B * k * H * W)
        outs = {key: guard((n + PAD,), torch.float32) for key, n in sizes.items()}
        info = torch.full((2 * G + PAD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        nbytes = L.gdf_op_pca_workspace(B, C_, H, W, k, int(joint))
        ws = torch.full((nbytes + TAIL,), PAT8, dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
        src = R.agg_src(d.data_ptr(), d.dtype == torch.float32, d.stride(), d.shape)
        torch.cuda.current_stream().synchronize()                            # the guard fills are done before another stream writes
        ok(L.gdf_op_pca(ctypes.addressof(src), B, k, int(joint), max_iter, tol, P(outs["mean"]), P(outs["components"]), P(outs["variance"]),
                        P(outs["total_variance"]), P(outs["projection"]) if projection else None, P(info), P(ws), nbytes, st), L)
        if size is not False and k == 3 and projection:
            OH, OW = R.out_size(H, W, size)
            rgb = torch.full((B * OH * OW * 3 + PAD,), PAT8, dtype=torch.uint8, device="cuda")
            ok(L.gdf_op_pca_rgb(P(outs["projection"]), B, H, W, int(joint), P(rgb), OH, OW, st), L)
        torch.cuda.synchronize()
        assert bool((ws[nbytes:].cpu() == PAT8).all()), "written behind the reported workspace size"
        info = info.cpu()
        assert bool((info[2 * G:] == 0x5A5A5A5A).all()), "written behind info"
        self.n_iter, self.converged = info[:2 * G].view(G, 2)[:, 0].numpy(), info[:2 * G].view(G, 2)[:, 1].numpy()
        shapes = dict(mean=(G, C_), components=(G, k, C_), variance=(G, k), total_variance=(G,), projection=(B, k, H, W))
        self.out = {}
        for key, n in sizes.items():
            o = outs[key].cpu()
            assert bool(is_guard(o[n:]).all()), "written behind " + key
            if key == "projection" and not projection:
                assert bool(is_guard(o).all())
                continue
            assert not bool(is_guard(o[:n]).any()), key + " not written"
            self.out[key] = o[:n].view(shapes[key]).numpy()
        if size is not False and k == 3 and projection:
            rgb = rgb.cpu()
            assert bool((rgb[B * OH * OW * 3:] == PAT8).all()), "written behind the picture"
            self.u8 = rgb[:B * OH * OW * 3].view(B, OH, OW, 3).numpy()
            # the normalised picture from the op's own projection, in float64: what the colour pass was given
            self.out["picture"] = R.colour(self.out["projection"], joint, None)["picture"]

    def same(self, other):
        keys = [k for k in self.out if k != "picture"]
        return all(torch.equal(bits(torch.from_numpy(self.out[k])), bits(torch.from_numpy(other.out[k]))) for k in keys) and \
            np.array_equal(self.u8, other.u8) and np.array_equal(self.n_iter, other.n_iter)


def run_case(name, layout=None):
    x, lay, joint, size, bd = R.case(name)
    r = Run(on_device(x, layout or lay), joint=joint, size=size)
    print("pca %s: iterations %s, converged %s" % (name, r.n_iter, r.converged))
    bd.check(r.out, what=name)
    bd.check_u8(r.u8, what=name)
    assert bool((r.converged == 1).all()) and bool((r.n_iter < R.MAX_ITER).all()) and bool((r.n_iter >= 1).all())
    return r, bd


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "independent B 2"])
def test_one_run_against_the_oracle(name):
    run_case(name)


def test_an_offset_view_with_a_longer_pixel_stride():
    run_case("C 96 on 24 x 24 channels-last", layout="view")


def test_independent_images_have_the_bits_of_their_own_call():
    x, lay, joint, size, bd = R.case("independent B 2")
    d = on_device(x, lay)
    both = Run(d)
    bd.check(both.out, what="independent B 2")
    bd.check_u8(both.u8, what="independent B 2")
    flipped = Run(torch.flip(d, (0,)).contiguous(memory_format=torch.channels_last))
    for b in range(2):
        one = Run(d[b:b + 1])
        for other, pos in ((both, b), (flipped, 1 - b)):
            for key in ("mean", "components", "variance", "total_variance", "projection"):
                assert np.array_equal(one.out[key][0].view(np.int32), other.out[key][pos].view(np.int32)), (b, pos, key)
            assert np.array_equal(one.u8[0], other.u8[pos]) and one.n_iter[0] == other.n_iter[pos]


def test_max_iter_2_reports_and_warns_once():
    from components.postproc import pca
    x = R.case("slow")[0]
    d = on_device(x, "nchw")
    r = Run(d, max_iter=2)                                                   # the guards behind every output are checked inside
    assert int(r.converged[0]) == 0 and int(r.n_iter[0]) == 2
    assert all(bool(np.isfinite(v).all()) for v in r.out.values())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = pca(d, max_iter=2)
    assert len(w) == 1 and "did not converge" in str(w[0].message)
    assert not bool(res.converged[0]) and int(res.n_iter[0]) == 2
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = pca(d)
    assert len(w) == 0 and bool(res.converged[0])


def test_the_same_bits_on_two_streams():
    x = R.case("C 77 on 16 x 16 NCHW")[0]
    d = on_device(x, "nchw")
    first = Run(d, size=32)
    again = Run(d, size=32)
    s1 = torch.cuda.Stream(priority=-1)                                      # (its own pool: the streams later tests draw are those they drew before)
    torch.cuda.synchronize()
    other = Run(d, size=32, st=vp(s1.cuda_stream))
    assert first.same(again) and first.same(other)


def test_a_zero_range_component_colours_0():
    """channel 2 is constant: the centred covariance has rank 2, the third direction does not exist, its projection is exactly constant"""
    x = R.features("planted", 1, 3, 6, 6, 21)
    x[:, 2] = 0.5
    r = Run(torch.from_numpy(x).cuda())
    want = R.oracle(x)
    assert bool((r.u8[..., 2] == 0).all())
    assert int(np.abs(r.u8[..., :2].astype(np.int32) - want["u8"][..., :2].astype(np.int32)).max()) <= 1
    assert float(np.ptp(r.out["projection"][0, 2])) == 0.0


def test_no_projection_leaves_the_rest_unchanged():
    x = R.case("C 96 on 24 x 24 channels-last")[0]
    d = on_device(x, "cl")
    r = Run(d, projection=False)                                             # (the untouched projection buffer is checked inside)
    full = Run(d)
    assert all(np.array_equal(r.out[k], full.out[k]) for k in r.out)


def test_k_8_against_the_oracle():
    """the API's limit on the geometric spectrum, whose eight leading eigenvalues are distinct: components 4 - 8 and their projections too"""
    x = R.case("geometric")[0]
    bd = R.Bounds(x, 8, False, None)
    r = Run(on_device(x, "cl"), k=8)
    print("pca geometric, k = 8: iterations %s, converged %s" % (r.n_iter, r.converged))
    assert r.out["projection"].shape == (1, 8, 24, 24)
    bd.check(r.out, what="geometric, k = 8")
    assert int(r.converged[0]) == 1 and int(r.n_iter[0]) < R.MAX_ITER


# ------------------------------------------------------------------------------------------------------------------------------
# Python level
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers_agree_with_the_c_calls():
    from components.postproc import pca, pca_rgb
    x, lay, joint, size, bd = R.case("8 x 20 to size 64")
    d = on_device(x, lay)
    r = Run(d, size=64)
    res = pca(d)
    assert res.projection.is_cuda and res.components.dtype == torch.float32
    assert np.array_equal(res.components.cpu().numpy(), r.out["components"]) and np.array_equal(res.projection.cpu().numpy(), r.out["projection"])
    assert np.array_equal(res.explained_variance.cpu().numpy(), r.out["variance"]) and int(res.n_iter[0]) == int(r.n_iter[0])
    ratio = res.explained_variance_ratio.cpu().numpy()
    assert np.allclose(ratio, r.out["variance"] / r.out["total_variance"][:, None], rtol=1e-6) and float(ratio.sum()) < 1.0
    pic = pca_rgb(d, 64)
    assert pic.is_cuda and pic.dtype == torch.uint8 and tuple(pic.shape) == (1, 64, 160, 3)
    assert np.array_equal(pic.cpu().numpy(), r.u8)
    assert tuple(pca_rgb(d, None).shape) == (1, 8, 20, 3)
    xj = R.case("joint B 2")[0]
    dj = on_device(xj, "nchw")
    assert np.array_equal(pca_rgb(dj, None, joint=True).cpu().numpy(), Run(dj, joint=True).u8)


def test_visualize_on_a_synthetic_sd15_extractor(monkeypatch):
    """the synthetic '1-5' extractor of tests/test_gpu_aggregate.py at its image size: an 8 x 8 hook of 1280 channels and a 32 x 32 one of 320"""
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    from components.postproc import pca_rgb
    from test_gpu_aggregate import LAYERS
    from test_gpu_glue import gen
    fe = diffusion_feature.FeatureExtractor(layer=dict(LAYERS), version="1-5", img_size=256, device="cuda:0")
    prompt = fe.encode_prompt("a photo of a cat")
    torch.manual_seed(0)
    feats = fe.extract(prompt, batch_size=2, image=torch.rand(2, 3, 256, 256, generator=gen(5)) * 2 - 1, image_type="tensors", t=100)
    pics = fe.visualize(size=32)
    assert list(pics) == list(feats)
    for k, v in feats.items():
        B, C_, H, W = v.shape
        assert pics[k].dtype == torch.uint8 and pics[k].is_cuda and tuple(pics[k].shape) == (B,) + R.out_size(H, W, 32) + (3,)
        assert torch.equal(pics[k], pca_rgb(v, 32))
        assert np.array_equal(pics[k].cpu().numpy(), Run(v, size=32).u8)                    # the op called directly
    some = list(feats)[:1]
    assert list(fe.visualize(feats, layers=some, size=None)) == some
    with pytest.raises(ValueError):
        fe.visualize(feats, layers=["no such layer"])
    assert callable(diffusion_feature.FeatureExtractor.visualize)
    del fe, feats, pics
    gc.collect()
    torch.cuda.synchronize()
