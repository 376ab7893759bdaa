"""Dense matching, the parts that need no GPU: the C symbols (declared, documented, exported, bound, every refusal on the host, the workspace
size), the host-tensor path of components/postproc.py dense_match / mutual_nn / dense_nn_correspondences against the float64 oracle of
tests/dense_match_ref.py and the reference's own results (tests/golden/dense_match.npz, written by tests/golden/gen_golden_dense.py), and the
ambiguity cap of the inputs that tests/test_gpu_dense_match.py uses."""
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

import dense_match_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_match.npz")


def _lib():
    import __graft_entry__ as G
    G.build()
    return R.bind(ctypes.CDLL(G.LIB))


def test_symbols_declared_documented_exported_and_bound():
    lib = _lib()
    src = open(os.path.join(ROOT, "include", "gdf_ops.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsize_t\s+gdf_op_dense_match_workspace\s*\(\s*int\s+B\s*,\s*int\s+C\s*,\s*int\s+P1\s*,\s*int\s+P2\s*,\s*int\s+f32_1\s*,"
                     r"\s*int\s+f32_2\s*\)", code)
    assert re.search(r"\bint\s+gdf_op_dense_match\s*\(\s*const\s+gdf_agg_src\s*\*\s*f1\s*,\s*const\s+gdf_agg_src\s*\*\s*f2\s*,\s*int\s+B\s*,"
                     r"\s*int\s*\*\s*nn12\s*,\s*float\s*\*\s*sim12\s*,\s*int\s*\*\s*nn21\s*,\s*float\s*\*\s*sim21\s*,\s*void\s*\*\s*workspace\s*,"
                     r"\s*size_t\s+workspace_bytes\s*,\s*void\s*\*\s*stream\s*\)", code)
    doc = src[:src.index("size_t gdf_op_dense_match_workspace")].rsplit("/*", 1)[1]
    for word in ("GDF_ERR_ARG", "GDF_ERR_UNSUPPORTED", "B == 0", "workspace", "NaN", "nn21", "sim21", "LOWEST", "same bits", "may be null"):
        assert word in doc, word
    assert hasattr(lib, "gdf_op_dense_match") and hasattr(lib, "gdf_op_dense_match_workspace") and lib.gdf_abi_version() == 1
    import __graft_entry__ as G
    assert "densematch.hip" in G.SOURCES and G.PER_FILE_FLAGS["densematch.hip"] == ["-fno-slp-vectorize"]
    kern = open(os.path.join(ROOT, "generic-diffusion-feature_amd", "csrc", "kernels.h")).read()
    assert "launch_dense_match" in kern and "dense_match_workspace" in kern
    from components import postproc
    res, args = postproc._SIG["gdf_op_dense_match"]
    assert res is ctypes.c_int and len(args) == len(R.DM_ARGTYPES) and postproc._SIG["gdf_op_dense_match_workspace"][0] is ctypes.c_size_t
    for fn in ("dense_match", "mutual_nn", "cycle_index", "dense_nn_correspondences", "find_best_buddies_correspondences"):
        assert callable(getattr(postproc, fn)), fn
    import diffusion_feature
    assert callable(diffusion_feature.FeatureExtractor.match)


def test_argument_errors_are_refused_on_the_host():
    """every refusal happens before any launch: the pointers are host memory that no kernel could touch, and there may be no device at all"""
    lib = _lib()
    big = lib.gdf_op_dense_match_workspace(2, 8, 16, 16, 0, 0)
    mem = (ctypes.c_char * 4096)()
    ptr = ctypes.addressof(mem)
    ptr += (-ptr) % 16

    def call(B=2, nn12=ptr, sim12=ptr, nn21=ptr, sim21=ptr, ws=ptr, ws_bytes=big, f1="s", f2="s", **over):
        s1 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        s2 = R.agg_src(ptr, 0, (128, 1, 32, 8), (B, 8, 4, 4))
        for k, v in over.items():
            setattr(s2 if k.endswith("2") else s1, k[:-1], v)
        return lib.gdf_op_dense_match(ctypes.addressof(s1) if f1 else None, ctypes.addressof(s2) if f2 else None, B, nn12, sim12, nn21, sim21, ws,
                                      ws_bytes, None)

    cases = [dict(f1=None), dict(f2=None), dict(ws=None), dict(ptr1=None), dict(ptr2=None), dict(C1=0, C2=0), dict(H1=0), dict(W1=0), dict(H2=0),
             dict(W2=-1), dict(C1=7), dict(C2=9), dict(ws_bytes=big - 1), dict(ws_bytes=0), dict(B=-1), dict(ws=ptr + 4),
             dict(nn12=None), dict(sim21=None), dict(nn12=None, sim12=None, nn21=None, sim21=None)]
    for kw in cases:
        assert call(**kw) == R.GDF_ERR_ARG, kw
        assert b"gdf_op_dense_match" in lib.gdf_last_error(), (kw, lib.gdf_last_error())
    # sizes the int32 indices and the grid cannot carry: refused as unsupported, not computed wrongly (checked before the workspace size)
    for kw in (dict(B=65536), dict(H1=1 << 16, W1=(1 << 14) + 1), dict(H2=1 << 15, W2=(1 << 15) + 1),
               dict(H1=1 << 12, W1=1 << 12, H2=1 << 12, W2=1 << 12)):
        assert call(**kw) == R.GDF_ERR_UNSUPPORTED, kw
        assert b"gdf_op_dense_match" in lib.gdf_last_error()
    assert call(B=0) == 0                                                  # B == 0: a successful no-op, checked after the arguments
    assert call(B=0, nn12=None, sim12=None) == 0 and call(B=0, nn21=None, sim21=None) == 0
    assert call(B=0, C2=9) == R.GDF_ERR_ARG and call(B=0, ws_bytes=0) == R.GDF_ERR_ARG
    assert not any(bytes(mem))                                             # nothing wrote to the 'device' memory


def test_workspace_size():
    lib = _lib()
    W = lib.gdf_op_dense_match_workspace
    base = dict(B=2, C=64, P1=300, P2=200, f32_1=0, f32_2=0)
    w0 = W(*base.values())
    assert w0 > 0 and W(1, 1, 1, 1, 0, 0) > 0 and W(0, 0, 0, 0, 0, 0) == W(1, 1, 1, 1, 0, 0)
    for k in ("B", "C", "P1", "P2"):
        prev = 0
        for v in (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 3520):
            w = W(*{**base, k: v}.values())
            assert w >= prev and w > 0, (k, v)
            prev = w
    assert W(2, 64, 300, 200, 1, 0) > w0 and W(2, 64, 300, 200, 0, 1) > w0 and W(2, 64, 300, 200, 1, 1) > W(2, 64, 300, 200, 1, 0)
    # the product's shape: two fp16 panels of 16384 x 3520 (2 x 110 MiB) and the tile partials (2 x 2 x 8 MiB), next to the 1 GiB matrix
    full = W(1, 3520, 16384, 16384, 0, 0)
    assert 2 * 16384 * 3520 * 2 <= full < 320 << 20
    # at least the operand panels: 2 bytes per element of an fp16 map, 4 of an fp32 map, padded
    assert W(1, 37, 323, 480, 1, 1) >= (512 + 512) * 64 * 4


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU cases: the ambiguity cap is a condition on them, checked here where no device is needed
# ------------------------------------------------------------------------------------------------------------------------------
def _white(C, g1, g2, f32, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(C, *g1, generator=g), torch.randn(C, *g2, generator=g)
    return (a.numpy(), b.numpy()) if f32 else (a.half().numpy(), b.half().numpy())


@pytest.mark.parametrize("C,g1,g2,f32", [(200, (40, 36), (33, 31), False), (72, (40, 36), (33, 31), False), (37, (17, 19), (24, 20), True)])
def test_white_noise_inputs_are_under_the_ambiguity_cap(C, g1, g2, f32):
    a, b = _white(C, g1, g2, f32, 7)
    S, tol = R.oracle(a, b), R.tolerance(C, 2 * int(f32))
    for T, cls, what in ((S, R.classes(b), "rows"), (S.T, R.classes(a), "columns")):
        share = R.ambiguous(T, tol, cls).mean()
        print("white noise %s C = %d: %.2f %% ambiguous %s" % ((g1, g2), C, 100 * share, what))
        assert share <= R.MAX_AMBIGUOUS


def planted(C=3520, P=512, seed=11):
    """b = a[perm] + 0.5 noise, rounded to fp16: (a, b) (C, P, 1) fp16 numpy and perm with b[:, q] ~ a[:, perm[q]]"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(C, P, generator=g).half()
    perm = torch.randperm(P, generator=g)
    b = (a.float()[:, perm] + 0.5 * torch.randn(C, P, generator=g)).half()
    return a.numpy()[:, :, None], b.numpy()[:, :, None], perm.numpy()


def test_planted_inputs_are_unambiguous():
    a, b, perm = planted()
    S, tol = R.oracle(a, b), R.tolerance(3520)
    assert not R.ambiguous(S, tol, R.classes(b)).any() and not R.ambiguous(S.T, tol, R.classes(a)).any()
    top = np.sort(S, axis=1)[:, -2:]
    assert top[:, 1].min() >= 0.88 and top[:, 0].max() <= 0.084
    inv = np.argsort(perm)
    assert np.array_equal(S.argmax(1), inv) and np.array_equal(S.argmax(0), perm)


# ------------------------------------------------------------------------------------------------------------------------------
# the host path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_host_dense_match_against_the_oracle(f32):
    from components.postproc import cycle_index, dense_match, mutual_nn
    g = torch.Generator().manual_seed(5)
    f1, f2 = torch.randn(2, 24, 9, 7, generator=g), torch.randn(2, 24, 6, 8, generator=g)
    f1, f2 = (f1, f2) if f32 else (f1.half(), f2.half())
    nn12, sim12, nn21, sim21 = dense_match(f1, f2)
    assert nn12.dtype == torch.int64 and nn21.dtype == torch.int64 and sim12.dtype == torch.float32 and sim21.dtype == torch.float32
    assert tuple(nn12.shape) == tuple(sim12.shape) == (2, 63) and tuple(nn21.shape) == tuple(sim21.shape) == (2, 48)
    for b in range(2):
        R.check(nn12[b].numpy(), sim12[b].numpy(), nn21[b].numpy(), sim21[b].numpy(), f1[b].numpy(), f2[b].numpy(), "host sample %d" % b,
                lowest_in_class=False)
    one = dense_match(f1, f2, "12")
    assert one[2] is None and one[3] is None and torch.equal(one[0], nn12)
    one = dense_match(f1, f2, "21")
    assert one[0] is None and one[1] is None and torch.equal(one[2], nn21)
    mask, m12, s12 = mutual_nn(f1, f2)
    assert mask.dtype == torch.bool and torch.equal(m12, nn12) and torch.equal(s12, sim12)
    assert torch.equal(mask, nn21.gather(1, nn12) == torch.arange(63)[None]) and torch.equal(cycle_index(nn12, nn21), nn21.gather(1, nn12))
    assert 0 < int(mask.sum()) < mask.numel()
    with pytest.raises(ValueError):
        dense_match(f1, f2[:, :8])
    with pytest.raises(ValueError):
        dense_match(f1, f2, "up")


def test_host_mutual_nn_saliency_conditions():
    from components.postproc import dense_match, mutual_nn
    g = torch.Generator().manual_seed(6)
    f1 = torch.randn(1, 16, 8, 8, generator=g)
    f2 = f1 + 0.4 * torch.randn(1, 16, 8, 8, generator=g)
    s1, s2 = torch.rand(1, 64, generator=g), torch.rand(1, 8, 8, generator=g)
    nn12, _, nn21, _ = dense_match(f1, f2)
    plain = mutual_nn(f1, f2)[0]
    want = plain.clone()
    want &= s1 > 0.3
    reached = torch.zeros(64, dtype=torch.bool)
    reached[nn21[0][s2.reshape(-1) > 0.3]] = True
    want &= reached[None]
    got = mutual_nn(f1, f2, s1, s2, thresh=0.3)[0]
    assert torch.equal(got, want) and 0 < int(got.sum()) < int(plain.sum())
    assert torch.equal(mutual_nn(f1, f2, s1, None, 0.3)[0], plain & (s1 > 0.3))


@pytest.mark.parametrize("name", ["nn_fp16", "nn_fp32"])
def test_host_tensors_equal_the_reference(name):
    from components.postproc import dense_match, dense_nn_correspondences
    z = np.load(GOLDEN)
    f1, f2 = torch.from_numpy(z[name + ":f1"]), torch.from_numpy(z[name + ":f2"])
    # the oracle accepts the reference's own answers
    R.check(z[name + ":nn12"][0], z[name + ":sim12"][0], z[name + ":nn21"][0], z[name + ":sim21"][0], f1[0].float().numpy(), f2[0].float().numpy(),
            "golden " + name, lowest_in_class=False)
    nn12, sim12, nn21, sim21 = dense_match(f1, f2)
    assert np.array_equal(nn12.numpy(), z[name + ":nn12"]) and np.array_equal(nn21.numpy(), z[name + ":nn21"])
    assert np.allclose(sim12.numpy(), z[name + ":sim12"], atol=1e-6) and np.allclose(sim21.numpy(), z[name + ":sim21"], atol=1e-6)
    p1, p2 = dense_nn_correspondences(f1, f2)
    assert p1.dtype == torch.float32 and p2.dtype == torch.float32
    assert np.array_equal(p1.numpy(), z[name + ":points1"]) and np.array_equal(p2.numpy(), z[name + ":points2"])
    with pytest.raises(ValueError):
        dense_nn_correspondences(f1, f2[:, :, :-1])


def test_host_best_buddies_equal_the_reference():
    pytest.importorskip("sklearn")
    from components.postproc import find_best_buddies_correspondences, mutual_nn
    z = np.load(GOLDEN)
    d1, d2, s1, s2 = (torch.from_numpy(z["bb:" + k]) for k in ("d1", "d2", "s1", "s2"))
    k, thresh = int(z["bb:args"][0]), float(z["bb:args"][1])
    f1, f2 = (d[:, 0].permute(0, 2, 1)[..., None] for d in (d1, d2))
    mask, nn12, sim12 = mutual_nn(f1, f2, s1, s2, thresh)
    assert np.array_equal(nn12[0].numpy(), z["bb:nn12"]) and np.array_equal(mask[0].numpy(), z["bb:mask"])
    assert np.allclose(sim12[0].numpy(), z["bb:sim12"], atol=1e-6)
    p1, p2 = find_best_buddies_correspondences(d1, d2, s1, s2, num_pairs=k, thresh=thresh)
    assert p1.dtype == torch.float32 and tuple(p1.shape) == (k, 2) == tuple(p2.shape)
    assert np.array_equal(p1.numpy(), z["bb:points1"]) and np.array_equal(p2.numpy(), z["bb:points2"])
    none = find_best_buddies_correspondences(d1, d2, torch.zeros_like(s1), s2, num_pairs=k, thresh=thresh)
    assert none == ([], [])
