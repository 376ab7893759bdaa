"""The correspondence loss, the parts that need no GPU: the C symbols (declared, documented, exported, bound, every refusal on the host, the
workspace size), the float64 oracle of tests/clip_loss_ref.py against the reference's own results (tests/golden/clip_loss.npz), the fp32 emulation
of the kernels' summation order against the bounds of every GPU case, the host-tensor path of components/postproc.py clip_loss /
compute_clip_loss including autograd, the rounding of the points and the ValueErrors."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clip_loss_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_loss.npz")
GOLDEN_CASES = ("c40_6x6", "smoothed_9x9", "f32_8x8")


def _lib():
    import __graft_entry__ as G
    G.build()
    return R.bind(ctypes.CDLL(G.LIB))


def _golden(name):
    z = np.load(GOLDEN)
    get = lambda k: z[name + ":" + k]  # noqa: E731
    return (torch.from_numpy(get("f1")), torch.from_numpy(get("f2")), get("source_points"), get("target_points"),
            tuple(int(v) for v in get("output_size")), torch.from_numpy(get("loss")), torch.from_numpy(get("grad_f1")), torch.from_numpy(get("grad_f2")))


def _golden_bounds(name):
    from components.postproc import points_to_idxs
    f1, f2, sp, tp, size, loss, g1, g2 = _golden(name)
    src = torch.from_numpy(points_to_idxs(sp, size).astype(np.int64))[None]
    tgt = torch.from_numpy(points_to_idxs(tp, size).astype(np.int64))[None]
    return R.Bounds(f1, f2, src, tgt), src, tgt


def test_symbols_declared_documented_exported_and_bound():
    lib = _lib()
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsize_t\s+gdf_op_clip_loss_workspace\s*\(\s*int\s+B\s*,\s*int\s+N\s*,\s*int\s+C\s*,\s*int\s+P1\s*,\s*int\s+P2\s*\)", code)
    assert re.search(r"\bint\s+gdf_op_clip_loss\s*\(\s*const\s+gdf_agg_src\s*\*\s*f1\s*,\s*const\s+gdf_agg_src\s*\*\s*f2\s*,\s*int\s+B\s*,"
                     r"\s*const\s+long\s+long\s*\*\s*src_idx\s*,\s*const\s+long\s+long\s*\*\s*tgt_idx\s*,\s*int\s+N\s*,\s*float\s+scale\s*,"
                     r"\s*float\s*\*\s*loss\s*,\s*float\s*\*\s*terms\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"\bint\s+gdf_op_clip_loss_backward\s*\(.*?const\s+float\s*\*\s*grad_loss\s*,\s*float\s*\*\s*grad_f1\s*,\s*float\s*\*\s*grad_f2\s*,"
                     r"\s*void\s*\*\s*workspace\s*,\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)", code, flags=re.S)
    doc = src[src.index("compute_clip_loss"):src.index("size_t gdf_op_clip_loss_workspace")]
    for word in ("logsumexp", "workspace", "GDF_ERR_ARG", "GDF_ERR_UNSUPPORTED", "NaN", "no atomics", "fixed order", "B == 0", "duplicates"):
        assert word.lower() in doc.lower(), word
    for name in ("gdf_op_clip_loss", "gdf_op_clip_loss_backward", "gdf_op_clip_loss_workspace"):
        assert hasattr(lib, name), name
    assert lib.gdf_abi_version() == 1
    from components import postproc
    assert postproc._SIG["gdf_op_clip_loss"] == (ctypes.c_int, R.FWD_ARGTYPES)
    assert postproc._SIG["gdf_op_clip_loss_backward"] == (ctypes.c_int, R.BWD_ARGTYPES)
    assert postproc._SIG["gdf_op_clip_loss_workspace"][0] is ctypes.c_size_t
    assert callable(postproc.clip_loss) and callable(postproc.compute_clip_loss)
    import diffusion_feature
    assert callable(diffusion_feature.FeatureExtractor.correspondence_loss)
    import __graft_entry__ as G
    assert "cliploss.hip" in G.SOURCES and G.PER_FILE_FLAGS["cliploss.hip"] == ["-fno-slp-vectorize"]


def test_argument_errors_are_refused_on_the_host():
    """every refusal happens before any launch: the pointers are host memory that no kernel could touch, and there may be no device at all"""
    lib = _lib()
    mem = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(mem)
    ptr += (-ptr) % 16
    big = lib.gdf_op_clip_loss_workspace(2, 3, 8, 16, 16)

    def call(back, B=2, N=3, scale=14.0, src=ptr, tgt=ptr, out=ptr, ws=ptr, ws_bytes=big, f1="s", f2="s", **over):
        s1 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        s2 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        for k, v in over.items():
            setattr(s2 if k.endswith("2") else s1, k[:-1], v)
        a1, a2 = ctypes.addressof(s1) if f1 else None, ctypes.addressof(s2) if f2 else None
        if back:
            return lib.gdf_op_clip_loss_backward(a1, a2, B, src, tgt, N, scale, out, ptr, ptr, ws, ws_bytes, None)
        return lib.gdf_op_clip_loss(a1, a2, B, src, tgt, N, scale, out, None, ws, ws_bytes, None)

    cases = [dict(f1=None), dict(f2=None), dict(src=None), dict(tgt=None), dict(out=None), dict(ws=None), dict(ptr1=None), dict(ptr2=None),
             dict(C1=0, C2=0), dict(H1=0), dict(W1=0), dict(H2=0), dict(W2=-1), dict(N=0), dict(N=-2), dict(C1=7), dict(C2=9),
             dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
             dict(ws_bytes=big - 1), dict(ws_bytes=0), dict(B=-1), dict(ws=ptr + 4)]
    for back, name in ((0, b"gdf_op_clip_loss"), (1, b"gdf_op_clip_loss_backward")):
        for kw in cases:
            assert call(back, **kw) == R.GDF_ERR_ARG, (back, kw)
            assert name in lib.gdf_last_error(), (kw, lib.gdf_last_error())
        assert call(back, H1=1 << 15, W1=1 << 15) == R.GDF_ERR_UNSUPPORTED            # 2^30 pixels
        assert call(back, B=0) == 0                                                    # B == 0: a successful no-op, checked after the arguments
        assert call(back, B=0, N=0) == R.GDF_ERR_ARG and call(back, B=0, ws_bytes=0) == R.GDF_ERR_ARG
    assert not any(bytes(mem))                                                         # nothing wrote to the 'device' memory


def test_workspace_is_monotone_and_small():
    lib = _lib()
    base = dict(B=2, N=20, C=64, P1=256, P2=256)
    w0 = lib.gdf_op_clip_loss_workspace(*base.values())
    assert w0 > 0 and lib.gdf_op_clip_loss_workspace(1, 1, 1, 1, 1) > 0
    for k in base:
        prev = 0
        for v in (1, 2, 3, 7, 8, 9, 16, 17, 24, 25, 48, 70, 128, 3520):
            w = lib.gdf_op_clip_loss_workspace(*{**base, k: v}.values())
            assert w >= prev and w > 0, (k, v)
            prev = w
    # the product's shape: queries, cos and partial sums of both directions, against 2 GiB of similarity matrices
    assert lib.gdf_op_clip_loss_workspace(1, 20, 3520, 128 * 128, 128 * 128) < 16 << 20


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_accepts_the_reference(name):
    f1, f2, sp, tp, size, loss, g1, g2 = _golden(name)
    bd, src, tgt = _golden_bounds(name)
    assert loss.dim() == 0 and g1.shape == f1.shape and g2.shape == f2.shape
    bd.check(loss[None], None, g1, g2, what="golden " + name)
    # the closed form of the gradient in the emulation, against the same oracle
    bd.check(*R.emulate(f1, f2, src, tgt), what="emulation on golden " + name)


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulated_summation_order_passes_every_gpu_case(name):
    f1, f2, src, tgt, bd = R.case(name)
    bd.check(*R.emulate(f1, f2, src, tgt), what="emulation, " + name)


def test_emulation_with_scale_100_on_identical_maps():
    f = R.features(1, 40, 6, 6, seed=5)
    idx = R.indices(1, 12, 36, 5, distinct=True)
    bd = R.Bounds(f, f, idx, idx, scale=100.0)
    loss, terms, g1, g2 = R.emulate(f, f, idx, idx, scale=100.0)
    bd.check(loss, terms, g1, g2, what="emulation, planted")
    assert bool(torch.isfinite(loss).all()) and float(loss) < np.log(36)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_host_tensors_against_oracle_and_golden(name):
    from components.postproc import clip_loss, compute_clip_loss
    f1, f2, sp, tp, size, want, w1, w2 = _golden(name)
    bd, src, tgt = _golden_bounds(name)
    a, b = f1.clone().float().requires_grad_(True), f2.clone().float().requires_grad_(True)
    net = types.SimpleNamespace(logit_scale=torch.ones([]) * np.log(1 / 0.07))
    loss = compute_clip_loss(net, a, b, sp, tp, size)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    bd.check(loss.detach()[None], None, a.grad, b.grad, what="host compute_clip_loss " + name)
    assert abs(float(loss.detach()) - float(want)) <= bd.b_loss
    for got, ref in ((a.grad, w1), (b.grad, w2)):
        assert float((got - ref).norm() / ref.norm()) < 2 * max(bd.b_g1, bd.b_g2)
    # None = the reference's initial logit_scale; a number works too; clip_loss on the indices gives the same value
    l2 = compute_clip_loss(None, f1, f2, sp, tp, size)
    l3 = compute_clip_loss(types.SimpleNamespace(logit_scale=float(np.log(1 / 0.07))), f1, f2, sp, tp, size)
    l4 = clip_loss(f1, f2, src[0], tgt[0])                                             # (N,) indices for B = 1
    assert tuple(l4.shape) == (1,) and l4.dtype == torch.float32
    for v in (l2, l3, l4[0]):
        assert abs(float(v) - float(loss.detach())) <= bd.b_loss


def test_host_batches():
    from components.postproc import clip_loss
    f1, f2, src, tgt, bd = R.case("two grids two types")
    a, b = f1.clone().requires_grad_(True), f2.float().clone().requires_grad_(True)
    loss = clip_loss(a, b, src, tgt)
    assert tuple(loss.shape) == (2,)
    loss.sum().backward()
    bd.check(loss.detach(), None, a.grad, b.grad, what="host, B = 2")


def test_point_rounding_clipping_and_non_square_sizes():
    from components.postproc import compute_clip_loss, points_to_idxs
    pts = np.array([[0.5, 1.5], [2.5, 3.5], [-3.0, -0.2], [40.0, 11.4], [11.5, 10.5], [7.49, 7.51]])
    assert points_to_idxs(pts, (12, 12)).tolist() == [0 * 12 + 2, 2 * 12 + 4, 0, 11 * 12 + 11, 12 * 12 - 2, 7 * 12 + 8]
    assert points_to_idxs(pts.astype(np.float32), (12, 12)).dtype == np.float32          # the points' own precision
    # the reference's formula verbatim on a non-square size: rows are clipped to and multiplied by output_size[1], columns clipped to output_size[0]
    assert points_to_idxs(np.array([[9.0, 9.0], [2.0, 3.0]]), (8, 6)).tolist() == [6 * 5 + 7, 6 * 2 + 3]
    g = torch.Generator().manual_seed(7)
    f = torch.randn(1, 8, 6, 8, generator=g)
    inside = np.array([[9.0, 9.0], [2.0, 3.0]])
    assert compute_clip_loss(None, f, f, inside, inside, (8, 6)).dim() == 0             # 37 < 48: follows the formula
    with pytest.raises(ValueError):
        compute_clip_loss(None, f, f, inside, inside, (6, 8))                           # 8 * 7 + 5 = 61 leaves the 6 x 8 map
    # the target is the source and the scale is large: the loss is small only if every point took its own pixel
    f = torch.randn(1, 32, 12, 12, generator=g)
    net = types.SimpleNamespace(logit_scale=torch.tensor(np.log(100.0)))
    assert float(compute_clip_loss(net, f, f, pts, pts, (12, 12))) < 1e-3


def test_value_errors():
    from components.postproc import clip_loss, compute_clip_loss
    g = torch.Generator().manual_seed(3)
    f1, f2 = torch.randn(2, 8, 4, 4, generator=g), torch.randn(2, 8, 5, 5, generator=g)
    idx = torch.zeros(2, 3, dtype=torch.int64)
    assert tuple(clip_loss(f1, f2, idx, idx).shape) == (2,)
    for bad in (lambda: clip_loss(f1, f2[:, :4], idx, idx), lambda: clip_loss(f1[0], f2[0], idx, idx), lambda: clip_loss(f1, f2[:1], idx, idx),
                lambda: clip_loss(f1, f2, idx[0], idx[0]), lambda: clip_loss(f1, f2, idx, idx[:, :2]), lambda: clip_loss(f1, f2, idx[:, :0], idx[:, :0]),
                lambda: clip_loss(f1, f2, idx.float(), idx.float()), lambda: clip_loss(f1, f2, idx, idx, scale=0.0),
                lambda: clip_loss(f1, f2, idx, idx, scale=float("nan")),
                lambda: compute_clip_loss(None, f1, f2, np.zeros((3, 2)), np.zeros((3, 2)), (4, 4)),          # B must be 1
                lambda: compute_clip_loss(None, f1[:1], f2[:1], np.zeros((3, 2)), np.zeros((2, 2)), (4, 4)),
                lambda: compute_clip_loss(None, f1[:1], f2[:1], np.zeros((3, 3)), np.zeros((3, 3)), (4, 4)),
                lambda: compute_clip_loss(None, f1[:1], f2[:1], np.full((3, 2), 4.0), np.zeros((3, 2)), (5, 5))):  # 24 leaves the 4 x 4 map
        with pytest.raises(ValueError):
            bad()
