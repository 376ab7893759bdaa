"""Nearest-neighbour correspondence, the parts that need no GPU: the C symbols (declared, exported, bound, every refusal on the host, the
workspace size), the host-tensor path of components/postproc.py nn_match / find_nn_source_correspondences against the reference's own results
(tests/golden/corres_nn.npz) and the float64 oracle of tests/correspond_ref.py, and the rounding of the points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generic-diffusion-feature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import correspond_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "corres_nn.npz")
CASES = ("x4", "ratio_10_3", "two_grids")


def _lib():
    import __graft_entry__ as G
    G.build()
    return R.bind(ctypes.CDLL(G.LIB))


def _golden(name):
    z = np.load(GOLDEN)
    L = tuple(int(v) for v in z[name + ":load_size"])
    return torch.from_numpy(z[name + ":f1"]), torch.from_numpy(z[name + ":f2"]), z[name + ":points"], L, z[name + ":points2"]


def test_symbols_declared_exported_and_bound():
    lib = _lib()
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsize_t\s+gdf_op_nn_match_workspace\s*\(\s*int\s+B\s*,\s*int\s+N\s*,\s*int\s+C\s*,\s*int\s+h2\s*,\s*int\s+w2\s*\)", code)
    assert re.search(r"\bint\s+gdf_op_nn_match\s*\(\s*const\s+gdf_agg_src\s*\*\s*f1\s*,\s*const\s+gdf_agg_src\s*\*\s*f2\s*,", code)
    assert hasattr(lib, "gdf_op_nn_match") and hasattr(lib, "gdf_op_nn_match_workspace") and lib.gdf_abi_version() == 1
    from components import postproc
    res, args = postproc._SIG["gdf_op_nn_match"]
    assert res is ctypes.c_int and len(args) == 12 and postproc._SIG["gdf_op_nn_match_workspace"][0] is ctypes.c_size_t
    assert callable(postproc.nn_match) and callable(postproc.find_nn_source_correspondences)
    import diffusion_feature
    assert callable(diffusion_feature.FeatureExtractor.correspond)


def test_argument_errors_are_refused_on_the_host():
    """every refusal happens before any launch: the pointers are host memory that no kernel could touch, and there may be no device at all"""
    lib = _lib()
    mem = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(mem)
    ptr += (-ptr) % 16
    big = lib.gdf_op_nn_match_workspace(2, 3, 8, 4, 4)

    def call(B=2, N=3, LH=16, LW=16, points=ptr, yx=ptr, score=ptr, ws=ptr, ws_bytes=big, f1="s", f2="s", **over):
        s1 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        s2 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        for k, v in over.items():
            setattr(s2 if k.endswith("2") else s1, k[:-1], v)
        return lib.gdf_op_nn_match(ctypes.addressof(s1) if f1 else None, ctypes.addressof(s2) if f2 else None, B, points, N, LH, LW, yx, score,
                                   ws, ws_bytes, None)

    cases = [dict(f1=None), dict(f2=None), dict(points=None), dict(yx=None), dict(score=None), dict(ws=None), dict(ptr1=None), dict(ptr2=None),
             dict(C1=0, C2=0), dict(H1=0), dict(W1=0), dict(H2=0), dict(W2=-1), dict(LH=0), dict(LW=0), dict(LW=-5), dict(N=0), dict(N=-2),
             dict(C1=7), dict(C2=9), dict(ws_bytes=big - 1), dict(ws_bytes=0), dict(B=-1), dict(ws=ptr + 4)]
    for kw in cases:
        assert call(**kw) == R.GDF_ERR_ARG, kw
        assert b"gdf_op_nn_match" in lib.gdf_last_error(), (kw, lib.gdf_last_error())
    assert call(B=0) == 0                                                  # B == 0: a successful no-op, checked after the arguments
    assert call(B=0, N=0) == R.GDF_ERR_ARG and call(B=0, ws_bytes=0) == R.GDF_ERR_ARG
    assert not any(bytes(mem))                                             # nothing wrote to the 'device' memory


def test_workspace_is_monotone_and_non_zero():
    lib = _lib()
    base = dict(B=2, N=20, C=64, h2=16, w2=16)
    w0 = lib.gdf_op_nn_match_workspace(*base.values())
    assert w0 > 0 and lib.gdf_op_nn_match_workspace(1, 1, 1, 1, 1) > 0
    for k in base:
        prev = 0
        for v in (1, 2, 3, 7, 8, 9, 16, 17, 24, 25, 48, 70, 128, 3520):
            w = lib.gdf_op_nn_match_workspace(*{**base, k: v}.values())
            assert w >= prev > -1 and w > 0, (k, v)
            prev = w
        assert lib.gdf_op_nn_match_workspace(*{**base, k: 4 * base[k]}.values()) >= w0
    # the product's shape: q + D + G + partials, a few MB next to the 3.7 GB the torch chain materialises
    assert lib.gdf_op_nn_match_workspace(1, 20, 3520, 128, 128) < 8 << 20


@pytest.mark.parametrize("name", CASES)
def test_oracle_accepts_the_reference(name):
    f1, f2, pts, L, want = _golden(name)
    amb = R.check(want, None, f1[0].float().numpy(), f2[0].float().numpy(), pts, *L, lowest_in_class=False, what="golden " + name)
    assert want.dtype == np.int64 and want.shape == (pts.shape[0], 2) and amb.shape == (pts.shape[0],)


@pytest.mark.parametrize("name", CASES)
def test_host_tensors_equal_the_reference(name):
    from components.postproc import find_nn_source_correspondences, nn_match
    f1, f2, pts, L, want = _golden(name)
    S, tol, cls = R.oracle(f1[0].float().numpy(), f2[0].float().numpy(), pts, *L)
    clear = ~R.ambiguous(S, tol, cls)
    p1, p2 = find_nn_source_correspondences(f1, f2, pts, None, L)
    assert p1.dtype == torch.float64 and np.array_equal(p1.numpy(), pts) and p2.dtype == torch.int64 and tuple(p2.shape) == want.shape
    R.check(p2.numpy(), None, f1[0].float().numpy(), f2[0].float().numpy(), pts, *L, lowest_in_class=False, what="host " + name)
    twin = R.classes(*L, *f2.shape[2:], twins=True)
    assert R.same_answer(p2.numpy(), want, cls, twin, L[1], clear) > len(pts) // 2
    yx, score = nn_match(f1, f2, torch.from_numpy(pts), L)                 # (N, 2) points for B = 1; the scores against the oracle too
    assert yx.dtype == torch.int64 and tuple(yx.shape) == (1,) + want.shape and score.dtype == torch.float32 and tuple(score.shape) == (1, len(pts))
    R.check(yx[0].numpy(), score[0].numpy(), f1[0].float().numpy(), f2[0].float().numpy(), pts, *L, lowest_in_class=False, what="host nn_match " + name)
    R.same_answer(yx[0].numpy(), want, cls, twin, L[1], clear)


def test_batches_and_rectangular_load_sizes_on_the_host():
    from components.postproc import nn_match
    g = torch.Generator().manual_seed(3)
    f1, f2 = torch.randn(2, 24, 5, 7, generator=g).half(), torch.randn(2, 24, 5, 7, generator=g).half()
    pts = torch.rand(2, 16, 2, generator=g, dtype=torch.float64) * torch.tensor([20.0, 28.0], dtype=torch.float64)
    yx, score = nn_match(f1, f2, pts, (20, 28))
    assert tuple(yx.shape) == (2, 16, 2) and tuple(score.shape) == (2, 16)
    for b in range(2):
        R.check(yx[b].numpy(), score[b].numpy(), f1[b].float().numpy(), f2[b].float().numpy(), pts[b].numpy(), 20, 28, lowest_in_class=False,
                what="host rectangular, sample %d" % b)
    with pytest.raises(ValueError):
        nn_match(f1, f2[:, :8], pts, (20, 28))
    with pytest.raises(ValueError):
        nn_match(f1, f2, pts[0], (20, 28))                                 # (N, 2) points with B = 2


def test_point_rounding_half_to_even_and_clipping():
    from components.postproc import nn_match
    idx = R.source_index(np.array([[0.5, 1.5], [2.5, 3.5], [-3.0, -0.2], [40.0, 23.4], [23.5, 22.5], [7.49, 7.51]]), 24, 24)
    assert idx.tolist() == [[0, 2], [2, 4], [0, 0], [23, 23], [23, 22], [7, 8]]
    # the target is the source: a point's nearest neighbour is its own pixel, so the answer shows the index nn_match took
    g = torch.Generator().manual_seed(5)
    f = torch.randn(1, 32, 12, 12, generator=g)
    pts = np.array([[0.5, 1.5], [2.5, 3.5], [-3.0, -0.2], [40.0, 11.4], [11.5, 10.5], [7.49, 7.51]])
    yx, score = nn_match(f, f, torch.from_numpy(pts), (12, 12))            # identity size: every pixel its own class
    assert yx[0].tolist() == [[0, 2], [2, 4], [0, 0], [11, 11], [11, 10], [7, 8]]
    assert np.allclose(score[0].numpy(), 1.0, atol=1e-5)
