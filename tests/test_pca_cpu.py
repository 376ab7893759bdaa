"""The PCA of feature maps, the parts that need no GPU: the float64 oracle of tests/pca_ref.py against scikit-learn and against the reference's own
PNG pixels (tests/golden/pca_vis.npz, made by tests/golden/gen_golden_pca.py), the committed cases' excluded zones, the centring guard, the
host-tensor path of components/postproc.py pca / pca_rgb, every refusal that needs no device, the header's symbols and the CLI on the CPU."""
import ctypes
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pca_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pca_vis.npz")
GOLDEN_CASES = ("c24_10x10", "c77_12x12")


def _lib():
    import __graft_entry__ as G
    G.build()
    return R.bind(ctypes.CDLL(G.LIB))


@pytest.mark.parametrize("C_,S,seed", [(48, 12, 1), (77, 16, 2)])
def test_oracle_agrees_with_scikit_learn(C_, S, seed):
    """both dimensions <= 500: scikit-learn takes its deterministic full solver"""
    sk = pytest.importorskip("sklearn.decomposition")
    x = R.features("planted", 1, C_, S, S, seed)
    f = x[0].astype(np.float64).reshape(C_, -1).T
    p = sk.PCA(n_components=3)
    t = p.fit(f).transform(f)
    want = R.oracle(x, size=None)
    assert float(np.abs(p.components_ - want["components"][0]).max()) <= 1e-12
    assert float(np.abs(p.explained_variance_ - want["variance"][0]).max()) <= 1e-12 * want["variance"][0, 0]
    assert float(np.abs(p.mean_ - want["mean"][0]).max()) <= 1e-12
    img = t.reshape(S, S, 3)
    img = (img - img.min(axis=(0, 1))) / (img.max(axis=(0, 1)) - img.min(axis=(0, 1)))
    assert np.array_equal((img * 255).astype(np.uint8), want["u8"][0])


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_and_host_path_equal_the_reference_pixels(name):
    from components.postproc import pca_rgb
    z = np.load(GOLDEN)
    x, png = z[name + ":x"], z[name + ":png"]
    assert x.dtype == np.float16 and png.shape == (512, 512, 3) and png.dtype == np.uint8
    bd = R.Bounds(x, 3, False, 512)
    assert not bool(bd.excluded().any())                                     # the seed search of gen_golden_pca.py
    assert np.array_equal(bd.want["u8"][0], png)
    assert np.array_equal(bd.ref["u8"][0], png)                              # the fp32 restatement too
    assert np.array_equal(pca_rgb(torch.from_numpy(x)).numpy()[0], png)


@pytest.mark.parametrize("name", list(R.CASES))
def test_committed_cases_keep_the_excluded_zone_small(name):
    x, layout, joint, size, bd = R.case(name)
    assert float(bd.excluded().mean()) < 0.01
    bd.check_u8(bd.ref["u8"], what="fp32 restatement, " + name)
    assert all(v > 0 for v in bd.bound.values())


def test_big_mean_guards_the_centring():
    """the covariance as Gram matrix minus n mu mu^T, in fp32, misses the bound this input sets; the centred restatement defines it"""
    x, layout, joint, size, bd = R.case("big mean")
    gram = R.errors(R.restate32(x, gram=True), bd.want)
    assert gram["components"] > bd.bound["components"] and gram["projection"] > bd.bound["projection"]
    assert float(np.abs(x.astype(np.float64).mean(axis=(0, 2, 3))).max()) > 8 * float(np.sqrt(bd.want["variance"][0, 0]))


def test_host_tensors_against_the_oracle():
    from components.postproc import PCAResult, pca, pca_rgb
    for name in ("C 20 on 5 x 7", "8 x 20 to size 64", "joint B 2", "independent B 2", "C 320 on 32 x 32 fp32"):
        x, layout, joint, size, bd = R.case(name)
        t = torch.from_numpy(x)
        if layout == "cl":
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        res = pca(t, joint=joint)
        assert isinstance(res, PCAResult) and res.components.dtype == torch.float32 and bool(res.converged.all()) and int(res.n_iter.sum()) == 0
        got = dict(mean=res.mean.numpy(), components=res.components.numpy(), variance=res.explained_variance.numpy(),
                   total_variance=(res.explained_variance[:, 0] / res.explained_variance_ratio[:, 0]).numpy(), projection=res.projection.numpy())
        err = R.errors(got, bd.want)
        scale = float(np.abs(bd.want["projection"]).max())
        assert err["components"] <= 2.0 ** -23 and err["projection"] <= 2.0 ** -22 * scale and err["variance"] <= 2.0 ** -23, (name, err)
        pic = pca_rgb(t, size, joint)
        assert pic.dtype == torch.uint8 and not pic.is_cuda
        bd.check_u8(pic.numpy(), what="host path, " + name)


def test_value_errors():
    from components.postproc import pca, pca_rgb
    x = torch.zeros(1, 8, 4, 4)
    for bad in (dict(n_components=0), dict(n_components=9), dict(max_iter=0), dict(max_iter=2000), dict(tol=-1.0), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            pca(x, **bad)
    with pytest.raises(ValueError):
        pca(torch.zeros(8, 4, 4))
    with pytest.raises(ValueError):
        pca(torch.zeros(1, 2, 4, 4))                                         # k = 3 > C
    with pytest.raises(ValueError):
        pca(torch.zeros(1, 8, 1, 3))                                         # k = 3 > n - 1
    assert pca(torch.randn(2, 8, 1, 2), joint=True).components.shape == (1, 3, 8)     # 4 samples when joint
    with pytest.raises(ValueError):
        pca_rgb(x, size=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert tuple(pca_rgb(torch.randn(1, 8, 4, 6), size=8).shape) == (1, 8, 12, 3)
        assert tuple(pca_rgb(torch.randn(1, 8, 6, 4), size=None).shape) == (1, 6, 4, 3)
    const = torch.randn(1, 3, 4, 4)
    const[:, 2] = 0.5                                                        # a third direction that does not exist: colour 0
    res = pca(const)
    assert bool((res.components[0, 2] == 0).all()) and float(res.explained_variance[0, 2]) == 0.0 and bool((res.projection[0, 2] == 0).all())
    assert bool((pca_rgb(const, None)[..., 2] == 0).all()) and int(pca_rgb(const, None)[..., :2].max()) == 255


def test_symbols_declared_documented_exported_and_bound():
    lib = _lib()
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsize_t\s+gdf_op_pca_workspace\s*\(\s*int\s+B\s*,\s*int\s+C\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*int\s+k\s*,\s*int\s+joint\s*\)", code)
    assert re.search(r"\bint\s+gdf_op_pca\s*\(\s*const\s+gdf_agg_src\s*\*\s*src\s*,\s*int\s+B\s*,\s*int\s+k\s*,\s*int\s+joint\s*,\s*int\s+max_iter\s*,"
                     r"\s*float\s+tol\s*,\s*float\s*\*\s*mean\s*,\s*float\s*\*\s*components\s*,\s*float\s*\*\s*variance\s*,\s*float\s*\*\s*total_variance\s*,"
                     r"\s*float\s*\*\s*projection\s*,\s*int\s*\*\s*info\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)",
                     code)
    assert re.search(r"\bint\s+gdf_op_pca_rgb\s*\(\s*const\s+float\s*\*\s*projection\s*,\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*int\s+joint\s*,"
                     r"\s*unsigned\s+char\s*\*\s*out\s*,\s*int\s+OH\s*,\s*int\s+OW\s*,\s*void\s*\*\s*stream\s*\)", code)
    doc = src[src.index("plot_pca"):src.index("size_t gdf_op_pca_workspace")]
    for word in ("n - 1", "largest magnitude", "centred", "hi, lo", "Rayleigh-Ritz", "Jacobi", "tol", "max_iter", "workspace", "GDF_ERR_ARG",
                 "GDF_ERR_UNSUPPORTED", "no atomics", "fixed order", "no grid-wide wait", "B == 0", "floor((o + 0.5) in / out)", "zero range"):
        assert word.lower() in doc.lower(), word
    for name in ("gdf_op_pca", "gdf_op_pca_rgb", "gdf_op_pca_workspace"):
        assert hasattr(lib, name), name
    from components import postproc
    assert postproc._SIG["gdf_op_pca"] == (ctypes.c_int, R.PCA_ARGTYPES)
    assert postproc._SIG["gdf_op_pca_rgb"] == (ctypes.c_int, R.RGB_ARGTYPES)
    assert postproc._SIG["gdf_op_pca_workspace"] == (ctypes.c_size_t, R.WS_ARGTYPES)
    import diffusion_feature
    assert callable(diffusion_feature.FeatureExtractor.visualize)
    import __graft_entry__ as G
    assert "pca.hip" in G.SOURCES and G.PER_FILE_FLAGS["pca.hip"] == ["-fno-slp-vectorize"]


def test_argument_errors_are_refused_on_the_host():
    """every refusal happens before any launch: the pointers are host memory that no kernel could touch, and there may be no device at all"""
    lib = _lib()
    mem = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(mem)
    ptr += (-ptr) % 16
    big = lib.gdf_op_pca_workspace(2, 8, 4, 4, 3, 0)
    assert big > 0 and lib.gdf_op_pca_workspace(2, 8, 4, 4, 3, 1) > 0

    def call(B=2, k=3, joint=0, max_iter=8, tol=1e-6, out=ptr, proj=ptr, info=ptr, ws=ptr, ws_bytes=big, src="s", **over):
        s = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        for key, v in over.items():
            setattr(s, key, v)
        return lib.gdf_op_pca(ctypes.addressof(s) if src else None, B, k, joint, max_iter, tol, out, out, out, out, proj, info, ws, ws_bytes, None)

    cases = [dict(src=None), dict(out=None), dict(info=None), dict(ws=None), dict(ptr=None), dict(C=0), dict(H=0), dict(W=-1), dict(B=-1),
             dict(k=0), dict(k=9), dict(k=8, C=7), dict(k=3, H=1, W=3), dict(joint=2), dict(max_iter=0), dict(max_iter=1025), dict(tol=-1.0),
             dict(tol=float("nan")), dict(tol=float("inf")), dict(ws_bytes=big - 1), dict(ws_bytes=0), dict(ws=ptr + 4)]
    for kw in cases:
        assert call(**kw) == R.GDF_ERR_ARG, kw
        assert b"gdf_op_pca" in lib.gdf_last_error(), (kw, lib.gdf_last_error())
    huge = lib.gdf_op_pca_workspace(2, 4096, 4, 4, 3, 0)
    assert call(C=4097, ws_bytes=huge) == R.GDF_ERR_UNSUPPORTED and call(H=1 << 15, W=1 << 15, ws_bytes=1 << 62) == R.GDF_ERR_UNSUPPORTED
    assert call(B=0) == 0 and call(proj=None, B=0) == 0                      # B == 0: a successful no-op, checked after the arguments
    assert call(B=0, k=0) == R.GDF_ERR_ARG

    def rgb(B=2, H=4, W=4, joint=0, OH=8, OW=8, p=ptr, out=ptr):
        return lib.gdf_op_pca_rgb(p, B, H, W, joint, out, OH, OW, None)
    for kw in (dict(p=None), dict(out=None), dict(B=-1), dict(H=0), dict(W=0), dict(OH=0), dict(OW=-3), dict(joint=5)):
        assert rgb(**kw) == R.GDF_ERR_ARG, kw
        assert b"gdf_op_pca_rgb" in lib.gdf_last_error()
    assert rgb(H=1 << 16, W=1 << 16) == R.GDF_ERR_UNSUPPORTED and rgb(B=0) == 0
    assert not any(bytes(mem))                                               # nothing wrote to the 'device' memory


def test_workspace_grows_with_batch_and_channels():
    """(the number of sample ranges, and so the size, is not monotone in H W)"""
    lib = _lib()
    base = dict(B=2, C=64, H=16, W=16, k=3, joint=0)
    for key in ("B", "C"):
        prev = 0
        for v in (1, 2, 3, 7, 8, 9, 16, 17, 48, 70, 128, 129, 1280):
            w = lib.gdf_op_pca_workspace(*{**base, key: v}.values())
            assert w >= prev and w > 0, (key, v)
            prev = w
    assert lib.gdf_op_pca_workspace(1, 1280, 128, 128, 3, 0) < 64 << 20


def test_cli_on_the_cpu(tmp_path):
    from PIL import Image
    from components.postproc import pca_rgb
    import feature_visualization as cli
    base = [R.features("planted", 1, 24, 8, 8, 31)[0], R.features("slow", 1, 16, 8, 8, 32)[0]]
    attn = np.abs(R.features("planted", 1, 2 * 2 * 5, 8, 8, 33)[0])              # two types x two groups x five tokens
    np.save(tmp_path / "f.npy", np.concatenate(base + [attn]))
    out = cli.main(["--input", str(tmp_path / "f.npy"), "--block_divide", "24", "16", "--have_attn", "--attn_type", "up_cross", "down_cross",
                    "--attn_len", "5", "--output", str(tmp_path / "vis"), "--task_name", "t", "--device", "cpu", "--size", "32"])
    assert out == str(tmp_path / "vis" / "t")
    tree = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    want = ["base/0.png", "base/1.png"]
    for t in ("up_cross", "down_cross"):
        want += [f"attn/{t}/{i}.png" for i in range(2)] + [f"attn/{t}/{i}/{j}.png" for i in range(2) for j in range(5)]
    assert tree == sorted(want)
    for i, m in enumerate(base):
        assert np.array_equal(np.array(Image.open(os.path.join(out, "base", f"{i}.png"))), pca_rgb(torch.from_numpy(m[None]), 32).numpy()[0])
    group = attn[10:15]                                                      # down_cross, group 0
    assert np.array_equal(np.array(Image.open(os.path.join(out, "attn", "down_cross", "0.png"))), pca_rgb(torch.from_numpy(group[None]), 32).numpy()[0])
    grey = np.array(Image.open(os.path.join(out, "attn", "down_cross", "0", "3.png")))
    assert grey.shape == (256, 256, 3) and int(grey.max()) >= 250 and np.array_equal(grey[..., 0], grey[..., 1])
    with pytest.raises(SystemExit):
        cli.main(["--input", str(tmp_path / "f.npy"), "--block_divide", "100", "--output", str(tmp_path / "x"), "--device", "cpu"])
