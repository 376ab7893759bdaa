"""Nearest-neighbour correspondence on the GPU (-m gpu): the kernels of csrc/corres.hip through gdf_op_nn_match (include/gdf_ops.h),
components/postproc.py nn_match / find_nn_source_correspondences and FeatureExtractor.correspond.

Kernel level: ONE gdf_op_nn_match call against the float64 oracle of tests/correspond_ref.py — the acceptance rule with its per-pixel tolerance
derived from the number formats, the duplicate-class rule and the <= 10 % ambiguity condition; no measured figure.  Inputs are seeded randn cast
to fp16 (or a 3 x 3 box-smoothed variant), points uniform over [-0.1 L, 1.1 L) with a few on .5.  Outputs and the workspace are guard-filled as in
tests/test_gpu_glue.py: the (B, N, 2) and (B, N) elements written, everything behind them and behind the reported workspace size untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import correspond_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, gen, guard, is_guard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT64, PAT8, TAIL = 0x7FDA7FDA7FDA7FDA, 0xA5, 4096


def _lib():
    return R.bind(lib())


def smooth(v):
    p = torch.nn.functional.pad(v.float(), (1, 1, 1, 1), mode="replicate")
    return torch.nn.functional.avg_pool2d(p, 3, stride=1).to(v.dtype)


def feats(B, C_, h, w, f32=False, chlast=False, seed=0, smoothed=False):
    v = torch.randn(B, C_, h, w, generator=gen(seed))
    v = smooth(v) if smoothed else v
    v = v if f32 else v.half()
    return _cl(v) if chlast else v.contiguous()


def points(B, N, LH, LW, seed=0):
    p = (torch.rand(B, N, 2, generator=gen(seed + 77)) * 1.2 - 0.1) * torch.tensor([float(LH), float(LW)])
    k = min(N, 6)
    p[:, :k] = torch.floor(p[:, :k]) + 0.5                                   # .5: half to even
    return p.float()


def launch(L, d1, d2, pts, LH, LW, st=None):
    """d1, d2, pts: device tensors -> (yx (B, N, 2) int64, score (B, N)) on the CPU after the guard checks"""
    B, N = pts.shape[:2]
    yx = torch.full((B * N * 2 + 64,), PAT64, dtype=torch.int64, device="cuda")
    sc = guard((B * N + 64,), torch.float32)
    nbytes = L.gdf_op_nn_match_workspace(B, N, d2.shape[1], d2.shape[2], d2.shape[3])
    ws = torch.full((nbytes + TAIL,), PAT8, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and pts.is_contiguous() and pts.dtype == torch.float32
    s1 = R.agg_src(d1.data_ptr(), d1.dtype == torch.float32, d1.stride(), d1.shape)
    s2 = R.agg_src(d2.data_ptr(), d2.dtype == torch.float32, d2.stride(), d2.shape)
    ok(L.gdf_op_nn_match(ctypes.addressof(s1), ctypes.addressof(s2), B, P(pts), N, LH, LW, P(yx), P(sc), P(ws), nbytes,
                         st if st is not None else stream()), L)
    torch.cuda.synchronize()
    yx, sc, ws = yx.cpu(), sc.cpu(), ws.cpu()
    assert bool((yx[B * N * 2:] == PAT64).all()) and bool(is_guard(sc[B * N:]).all()), "written behind the outputs"
    assert not bool(is_guard(sc[:B * N]).any()) and not bool((yx[:B * N * 2] == PAT64).any()), "owned outputs not written"
    assert bool((ws[nbytes:] == PAT8).all()), "written behind the reported workspace size"
    return yx[:B * N * 2].view(B, N, 2), sc[:B * N].view(B, N)


def run(f1, f2, pts, LH, LW, what="", st=None):
    """host tensors (their strides are kept on the device) -> one call, every sample checked against the oracle"""
    L = _lib()
    d1, d2 = f1.cuda(), f2.cuda()
    assert d1.stride() == f1.stride() and d2.stride() == f2.stride()
    yx, sc = launch(L, d1, d2, pts.cuda(), LH, LW, st)
    for b in range(pts.shape[0]):
        R.check(yx[b].numpy(), sc[b].numpy(), f1[b].float().numpy(), f2[b].float().numpy(), pts[b].double().numpy(), LH, LW,
                what="%s, sample %d" % (what, b))
    return yx, sc


# C, (h1, w1), fp32 source, source channels-last, (h2, w2), fp32 target, target channels-last, (LH, LW), N, B, smoothed
CASES = {
    "x4 NCHW fp16": (40, (6, 6), 0, 0, (6, 6), 0, 0, (24, 24), 64, 2, 0),                  # the product's ratio; three query chunks (24 + 24 + 16)
    "channels-last non-square": (72, (5, 7), 0, 1, (5, 7), 0, 1, (24, 20), 64, 2, 0),       # non-integer ratios, C no multiple of 64, lanes along C
    "fp32 single query": (8, (16, 16), 1, 0, (16, 16), 1, 0, (64, 64), 1, 1, 0),            # four 64-pixel blocks, the 4-query instantiation
    "two grids two types": (136, (9, 9), 1, 0, (12, 12), 0, 1, (48, 48), 70, 2, 0),         # 70 = 24 + 24 + 22: across the chunk boundary
    "identity": (40, (8, 8), 0, 0, (8, 8), 0, 0, (8, 8), 32, 2, 0),                         # every lambda is 0; chunks of 24 and 8
    "ratio 10/3 smoothed": (16, (9, 9), 0, 0, (9, 9), 0, 0, (30, 30), 64, 2, 1),            # 81 coarse pixels: a partial 64-pixel block
    "one row": (40, (1, 9), 0, 0, (1, 9), 0, 0, (4, 12), 8, 2, 0),                          # i1 clamps everywhere on one axis
    "one column": (40, (9, 1), 0, 1, (9, 1), 0, 1, (12, 4), 8, 2, 0),
    "fp32 channels-last": (20, (7, 5), 1, 1, (7, 5), 1, 1, (21, 20), 12, 2, 0),             # 4 floats per lane; the 12-query instantiation
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_against_the_oracle(name):
    C_, g1, s32, scl, g2, t32, tcl, (LH, LW), N, B, sm = CASES[name]
    seed = sum(map(ord, name))
    f1 = feats(B, C_, *g1, f32=bool(s32), chlast=bool(scl), seed=seed, smoothed=bool(sm))
    f2 = feats(B, C_, *g2, f32=bool(t32), chlast=bool(tcl), seed=seed + 1, smoothed=bool(sm))
    run(f1, f2, points(B, N, LH, LW, seed), LH, LW, name)


def test_planted_shift_is_found_exactly():
    """the target is the source rolled by (2, -1) coarse pixels: a point whose taps do not wrap has its own vector at (y + 8, x - 4)"""
    B, C_ = 2, 40
    f1 = feats(B, C_, 8, 8, seed=21)
    f2 = torch.roll(f1, shifts=(2, -1), dims=(2, 3)).contiguous()
    ys, xs = [2, 5, 9, 13, 21], [6, 10, 17, 29]
    pts = torch.tensor([[float(y), float(x)] for y in ys for x in xs])[None].expand(B, -1, -1).contiguous()
    L = _lib()
    yx, sc = launch(L, f1.cuda(), f2.cuda(), pts.cuda(), 32, 32)
    want = (pts + torch.tensor([8.0, -4.0])).long()
    for b in range(B):
        amb = R.check(yx[b].numpy(), sc[b].numpy(), f1[b].float().numpy(), f2[b].float().numpy(), pts[b].double().numpy(), 32, 32,
                      what="planted shift, sample %d" % b)
        assert not amb.any()
        _, tol, _ = R.oracle(f1[b].float().numpy(), f2[b].float().numpy(), pts[b].double().numpy(), 32, 32)
        p = (want[b, :, 0] * 32 + want[b, :, 1]).numpy()
        assert (sc[b].numpy() >= 1.0 - tol[p] - 2.0 ** -23).all()
    assert torch.equal(yx, want)


def test_strided_views_keep_the_nan_padding_out():
    """both maps are views into larger NaN-filled buffers: x stride 2 inside an NCHW buffer (the any-stride path), and a channels-last buffer
    whose pixels are 8 channels longer than C (lanes along C must stop at C)"""
    B, C_, h, w, LH, LW, N = 2, 24, 6, 5, 18, 20, 16
    v1, v2 = feats(B, C_, h, w, seed=31), feats(B, C_, h, w, seed=32)
    pts = points(B, N, LH, LW, 33)
    L = _lib()

    def nchw_view(v):
        buf = torch.full((B, C_ + 3, h + 2, 2 * w + 1), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, 1:C_ + 1, 1:h + 1, 1:2 * w:2]
        view.copy_(v)
        return buf, view

    def cl_view(v):
        buf = torch.full((B, h + 1, w + 2, C_ + 8), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, :h, 1:w + 1, :C_].permute(0, 3, 1, 2)
        view.copy_(v)
        return buf, view

    for what, mk in (("x stride 2", nchw_view), ("padded channels-last pixels", cl_view)):
        b1, d1 = mk(v1)
        b2, d2 = mk(v2)
        assert tuple(d2.shape) == (B, C_, h, w) and not d2.is_contiguous() and bool(torch.isnan(b2).any())
        yx, sc = launch(L, d1, d2, pts.cuda(), LH, LW)
        assert bool(torch.isfinite(sc).all())
        for b in range(B):
            R.check(yx[b].numpy(), sc[b].numpy(), v1[b].float().numpy(), v2[b].float().numpy(), pts[b].double().numpy(), LH, LW,
                    what="%s, sample %d" % (what, b))


def test_streams_layouts_and_determinism():
    B, C_, LH, LW, N = 2, 48, 28, 28, 30
    f1, f2 = feats(B, C_, 7, 7, seed=41), feats(B, C_, 7, 7, seed=42)
    pts = points(B, N, LH, LW, 43)
    L = _lib()
    d1, d2, dp = f1.cuda(), f2.cuda(), pts.cuda()
    first = launch(L, d1, d2, dp, LH, LW)
    again = launch(L, d1, d2, dp, LH, LW)
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = launch(L, d1, d2, dp, LH, LW, st=vp(s1.cuda_stream))
    for got in (again, other):                                               # the same inputs: the same bits, on any stream
        assert torch.equal(got[0], first[0]) and torch.equal(got[1].view(torch.int32), first[1].view(torch.int32))
    run(f1, f2, pts, LH, LW, "NCHW copy")
    run(_cl(f1), _cl(f2), pts, LH, LW, "channels-last copy")                 # accepted too; equality between the two is not required


def test_beside_a_gemm_on_a_second_stream_keeps_its_bits():
    """one call while a GEMM runs on a second stream: the bits equal the solo run.  Once, no loop."""
    B, C_, LH, LW, N = 2, 320, 64, 64, 20
    L = _lib()
    d1, d2 = feats(B, C_, 16, 16, seed=61).cuda(), feats(B, C_, 16, 16, seed=62).cuda()
    dcl, dp = _cl(d2), points(B, N, LH, LW, 63).cuda()
    solo, solo_cl = launch(L, d1, d2, dp, LH, LW), launch(L, d1, dcl, dp, LH, LW)
    M = K = 4096
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    Wt = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    o16 = torch.zeros(M, M, dtype=torch.half, device="cuda")
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(6):                                                       # a few milliseconds of GEMM queued on s1, then the two calls on s0
        ok(L.gdf_op_gemm(P(A), K, P(Wt), None, None, None, 0, P(o16), M, None, 0, M, M, K, 0, vp(s1.cuda_stream)), L)
    beside = launch(L, d1, d2, dp, LH, LW, st=vp(s0.cuda_stream))
    beside_cl = launch(L, d1, dcl, dp, LH, LW, st=vp(s0.cuda_stream))
    for got, want in ((beside, solo), (beside_cl, solo_cl)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert bool(torch.isfinite(o16.float()).all())


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    d = feats(2, 8, 4, 4).cuda()
    pts = points(2, 3, 16, 16).cuda()
    yx = torch.full((12,), PAT64, dtype=torch.int64, device="cuda")
    sc = guard((6,), torch.float32)
    nbytes = L.gdf_op_nn_match_workspace(2, 3, 8, 4, 4)
    ws = torch.full((nbytes,), PAT8, dtype=torch.uint8, device="cuda")
    s1, s2 = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape), R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def call(B=2, N=3, LH=16, nb=nbytes):
        return L.gdf_op_nn_match(ctypes.addressof(s1), ctypes.addressof(s2), B, P(pts), N, LH, 16, P(yx), P(sc), P(ws), nb, stream())
    assert call(N=0) == R.GDF_ERR_ARG and call(LH=0) == R.GDF_ERR_ARG and call(nb=nbytes - 1) == R.GDF_ERR_ARG
    assert b"gdf_op_nn_match" in L.gdf_last_error()
    s2.C = 9
    assert call() == R.GDF_ERR_ARG
    s2.C = 8
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert bool((yx.cpu() == PAT64).all()) and bool(is_guard(sc.cpu()).all()) and bool((ws.cpu() == PAT8).all())


# ------------------------------------------------------------------------------------------------------------------------------
# Python level
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers_agree_with_the_c_call():
    import diffusion_feature
    from components.postproc import find_nn_source_correspondences, nn_match
    B, C_, LH, LW, N = 2, 40, 24, 24, 30
    f1, f2 = feats(B, C_, 6, 6, seed=51), feats(B, C_, 6, 6, chlast=True, seed=52)
    pts = points(B, N, LH, LW, 53)
    d1, d2 = f1.cuda(), f2.cuda()
    want = launch(_lib(), d1, d2, pts.cuda(), LH, LW)
    yx, sc = nn_match(d1, d2, pts, (LH, LW))                                 # host points are moved; the result stays on the device
    assert yx.is_cuda and sc.is_cuda and yx.dtype == torch.int64 and sc.dtype == torch.float32
    assert torch.equal(yx.cpu(), want[0]) and torch.equal(sc.cpu().view(torch.int32), want[1].view(torch.int32))
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    yx2, sc2 = fe.correspond(d1, d2, pts.cuda(), (LH, LW))
    assert torch.equal(yx2, yx) and torch.equal(sc2.view(torch.int32), sc.view(torch.int32))
    src = pts[0].double().numpy()
    p1, p2 = find_nn_source_correspondences(d1[:1], d2[:1], src, (6, 6), (LH, LW))
    assert p1.dtype == torch.float64 and np.array_equal(p1.numpy(), src)     # the reference's types and shapes
    assert p2.dtype == torch.int64 and tuple(p2.shape) == (N, 2) and torch.equal(p2.cpu(), want[0][0])


@pytest.mark.parametrize("name", ["x4", "ratio_10_3", "two_grids"])
def test_reference_results_on_the_device(name):
    from components.postproc import find_nn_source_correspondences
    z = np.load(os.path.join(ROOT, "tests", "golden", "corres_nn.npz"))
    f1, f2, pts, want = torch.from_numpy(z[name + ":f1"]), torch.from_numpy(z[name + ":f2"]), z[name + ":points"], z[name + ":points2"]
    LH, LW = (int(v) for v in z[name + ":load_size"])
    _, p2 = find_nn_source_correspondences(f1.cuda(), f2.cuda(), pts, None, (LH, LW))
    p2 = p2.cpu().numpy()
    a1, a2 = f1[0].float().numpy(), f2[0].float().numpy()
    R.check(p2, None, a1, a2, pts, LH, LW, what="golden on the device, " + name)
    S, tol, cls = R.oracle(a1, a2, pts, LH, LW)
    clear = ~R.ambiguous(S, tol, cls)
    assert R.same_answer(p2, want, cls, R.classes(LH, LW, *f2.shape[2:], twins=True), LW, clear) > len(pts) // 2
