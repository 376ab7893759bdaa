"""Bilinear aggregation of hooked features on the GPU (-m gpu): aggregate_kernel of csrc/post.hip through gdf_op_aggregate (include/gdf_ops.h),
components/postproc.py aggregate, FeatureExtractor.aggregate and the CLI's --aggregate_mode / --aggregate_size.

Kernel level: ONE gdf_op_aggregate call against the float64 reference of tests/aggregate_ref.py (fp32 coordinates as ATen defines them, float64
blend) under the bound derived there from the number formats — no measured figure.  Inputs are seeded randn, B = 2; every destination is
guard-filled as in tests/test_gpu_glue.py: owned elements written, everything else untouched."""
import os
import sys

import numpy as np
import pytest
import torch

from aggregate_ref import AggSrc, bind, check
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, assert_bits, assert_owned, gen, guard, is_guard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2


def _lib():
    return bind(lib())


def _src(C_, H, W, f32=False, chlast=True, seed=0):
    v = torch.randn(B, C_, H, W, generator=gen(seed))
    v = v if f32 else v.half()
    return _cl(v) if chlast else v.contiguous()


def _launch(L, vs, coffs, out, Ctot, OH, OW, mode=1, st=None):
    """vs: device tensors (kept alive by the caller); one gdf_op_aggregate call"""
    srcs = (AggSrc * len(vs))()
    for s, v, coff in zip(srcs, vs, coffs):
        s.ptr, s.f32 = v.data_ptr(), int(v.dtype == torch.float32)
        s.sb, s.sc, s.sy, s.sx = v.stride()
        _, s.C, s.H, s.W = v.shape
        s.coff = coff
    ok(L.gdf_op_aggregate(srcs, len(vs), B, P(out), int(out.dtype == torch.float32), Ctot, OH, OW, mode, st if st is not None else stream()), L)


def _run(vs, OH, OW, out_f32=False, coffs=None, Ctot=None, what=""):
    """one launch over the host tensors `vs` -> checks the guards and the bound of every source's channel range; returns the output on the CPU"""
    L = _lib()
    if coffs is None:
        coffs = list(np.cumsum([0] + [v.shape[1] for v in vs[:-1]]))
    Ctot = Ctot or sum(v.shape[1] for v in vs)
    out = guard((B, Ctot, OH, OW), torch.float32 if out_f32 else torch.float16)
    dev = [v.cuda() for v in vs]
    assert all(d.stride() == v.stride() for d, v in zip(dev, vs))
    _launch(L, dev, coffs, out, Ctot, OH, OW)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(got.shape, dtype=torch.bool)
    for v, coff in zip(vs, coffs):
        owned[:, coff:coff + v.shape[1]] = True
    assert_owned(got, owned)
    for v, coff in zip(vs, coffs):
        check(got[:, coff:coff + v.shape[1]].double().numpy(), v.float().numpy(), OH, OW, out_f32, what)
    return got


@pytest.mark.parametrize("H,W,C_,f32,chlast,OH,OW,out_f32,coff,Ctot", [
    (8, 8, 8, 0, 1, 16, 16, 0, 0, 8),            # x2: weights 1/4 and 3/4, 16-byte stores
    (12, 20, 70, 0, 1, 30, 30, 0, 5, 79),        # non-square, non-integer ratio, a full and a partial 64-channel chunk, OW % 8 != 0 and row starts that
                                                 # are not 16-byte aligned (scalar stores), foreign channels untouched
    (20, 136, 16, 1, 0, 200, 200, 0, 0, 16),     # a source row wider than one LDS slab; fp32 NCHW source (sc = H W)
    (192, 192, 8, 0, 1, 160, 160, 0, 0, 8),      # downsampling: the taps skip source pixels; two slabs
    (1, 9, 8, 0, 1, 4, 4, 0, 0, 8),              # i1 clamps on a one-pixel axis
    (9, 1, 8, 0, 1, 4, 4, 0, 0, 8),
    (16, 16, 8, 0, 1, 24, 40, 0, 0, 8),          # rectangular output
    (8, 8, 8, 0, 1, 16, 16, 1, 0, 8),            # fp32 output and its guards
    (8, 8, 8, 0, 1, 15, 18, 1, 3, 14)])          # fp32 output, scalar stores (OW % 4 != 0), foreign channels
def test_bilinear_one_source(H, W, C_, f32, chlast, OH, OW, out_f32, coff, Ctot):
    _run([_src(C_, H, W, bool(f32), bool(chlast), seed=H * 1000 + W)], OH, OW, bool(out_f32), [coff], Ctot, "one source")


@pytest.mark.parametrize("f32,chlast,out_f32", [(0, 1, 0), (1, 0, 0), (1, 1, 1)])
def test_identity_is_the_cast_source_bit_for_bit(f32, chlast, out_f32):
    L = _lib()
    v = _src(8, 53, 53, bool(f32), bool(chlast), seed=53)
    dt = torch.float32 if out_f32 else torch.float16
    out = guard((B, 11, 53, 53), dt)
    vd = v.cuda()
    _launch(L, [vd], [2], out, 11, 53, 53)
    torch.cuda.synchronize()
    want = guard((B, 11, 53, 53), dt, "cpu")
    want[:, 2:10] = v.to(dt)
    assert_bits(out, want)


def test_three_sources_in_one_call():
    """offsets and order in one launch, mixed layouts and source types"""
    vs = [_src(1280, 8, 8, seed=1), _src(320, 32, 32, seed=2), _src(77, 16, 16, f32=True, chlast=False, seed=3)]
    got = _run(vs, 32, 32, what="three sources")
    assert torch.equal(got[:, 1280:1600], vs[1].contiguous())                      # 32^2 -> 32^2: the hook itself


def test_more_sources_than_one_launch_takes():
    from components.postproc import aggregate
    vs = [_src(8, 4, 4, seed=100 + i) for i in range(20)]
    got = aggregate([v.cuda() for v in vs], 8)
    torch.cuda.synchronize()
    got = got.cpu()
    assert tuple(got.shape) == (B, 160, 8, 8) and got.dtype == torch.float16
    for i, v in enumerate(vs):
        check(got[:, 8 * i:8 * i + 8].double().numpy(), v.float().numpy(), 8, 8, False, "source %d of 20" % i)
    got32 = aggregate([v.cuda() for v in vs[:3]], (6, 10), dtype=torch.float32).cpu()
    assert got32.dtype == torch.float32 and tuple(got32.shape) == (B, 24, 6, 10)
    for i, v in enumerate(vs[:3]):
        check(got32[:, 8 * i:8 * i + 8].double().numpy(), v.float().numpy(), 6, 10, True, "fp32 source %d" % i)


@pytest.mark.parametrize("H,W,S,Cc,f32,chlast,coff,extra", [                      # the shapes of test_gpu_glue.py test_resize_concat
    (20, 136, 200, 16, 0, 1, 0, 0), (192, 192, 160, 8, 0, 1, 0, 0), (53, 53, 53, 8, 0, 1, 0, 0), (20, 136, 200, 70, 1, 0, 5, 9),
    (12, 20, 30, 70, 0, 1, 5, 9)])
def test_nearest_has_the_bits_of_resize_concat(H, W, S, Cc, f32, chlast, coff, extra):
    L = _lib()
    v = _src(Cc, H, W, bool(f32), bool(chlast), seed=H + S).cuda()
    Ctot = Cc + extra
    out, want = guard((B, Ctot, S, S), torch.float16), guard((B, Ctot, S, S), torch.float16)
    _launch(L, [v], [coff], out, Ctot, S, S, mode=0)
    sb, sc, sy, sx = v.stride()
    ok(L.gdf_op_resize_concat(P(v), f32, sb, sc, sy, sx, B, Cc, H, W, P(want), Ctot, coff, S, stream()), L)
    torch.cuda.synchronize()
    assert_bits(out, want.cpu())
    assert not bool(is_guard(out.cpu()[:, coff:coff + Cc]).any())


def test_device_refusals_launch_nothing():
    L = _lib()
    v = _src(8, 4, 4).cuda()
    out = guard((B, 10, 8, 8), torch.float16)
    srcs = (AggSrc * 1)()
    s = srcs[0]
    s.ptr, s.f32, s.C, s.H, s.W, s.coff = v.data_ptr(), 0, 8, 4, 4, 3
    s.sb, s.sc, s.sy, s.sx = v.stride()
    assert L.gdf_op_aggregate(srcs, 1, B, P(out), 0, 10, 8, 8, 1, stream()) != 0 and b"gdf_op_aggregate" in L.gdf_last_error()
    s.coff = 0
    assert L.gdf_op_aggregate(srcs, 1, B, P(out), 0, 10, 8, 8, 3, stream()) != 0
    assert L.gdf_op_aggregate(srcs, 1, 0, P(out), 0, 10, 8, 8, 1, stream()) == 0            # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


def test_beside_a_gemm_on_a_second_stream_keeps_its_bits():
    """one launch while a GEMM runs on a second stream: the bits equal the solo run.  Once, no loop."""
    L = _lib()
    vs = [_src(640, 16, 16, seed=11).cuda(), _src(320, 32, 32, seed=12).cuda()]
    solo, beside = guard((B, 960, 64, 64), torch.float16), guard((B, 960, 64, 64), torch.float16)
    _launch(L, vs, [0, 640], solo, 960, 64, 64)
    M = N = K = 4096
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    Wt = (torch.randn(N, K, generator=g) * 0.1).half().cuda()
    o16 = torch.zeros(M, N, dtype=torch.half, device="cuda")
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(4):                                                          # a few milliseconds of GEMM queued on s1, then the aggregation on s0
        ok(L.gdf_op_gemm(P(A), K, P(Wt), None, None, None, 0, P(o16), N, None, 0, M, N, K, 0, vp(s1.cuda_stream)), L)
    _launch(L, vs, [0, 640], beside, 960, 64, 64, st=vp(s0.cuda_stream))
    torch.cuda.synchronize()
    assert_bits(beside, solo.cpu())
    assert not bool(is_guard(solo.cpu()).any()) and bool(torch.isfinite(o16.float()).all())


# ------------------------------------------------------------------------------------------------------------------------------
# product level: the synthetic '1-5' extractor of tests/test_gpu_cli.py
# ------------------------------------------------------------------------------------------------------------------------------
LAYERS = {"up-level1-repeat2-res-out": True, "up-level3-repeat0-vit-block0-self-k": True}


def test_feature_extractor_aggregate(monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    import diffusion_feature
    from components.postproc import aggregate
    df = diffusion_feature.FeatureExtractor(layer=dict(LAYERS), version="1-5", img_size=256, device="cuda:0")
    prompt = df.encode_prompt("a photo of a cat")
    img = torch.rand(B, 3, 256, 256, generator=gen(5)) * 2 - 1
    torch.manual_seed(0)
    feats = df.extract(prompt, batch_size=B, image=img, image_type="tensors", t=100)
    assert list(feats) == list(LAYERS)
    got = df.aggregate(size=32)                                                  # the dict of the last extract()
    assert tuple(got.shape) == (B, 1600, 32, 32) and got.dtype == torch.float16
    assert torch.equal(got, aggregate(list(feats.values()), 32)) and torch.equal(got, df.aggregate(feats, size=32))
    hooks = [v.float().cpu() for v in feats.values()]
    got = got.cpu()
    check(got[:, :1280].double().numpy(), hooks[0].numpy(), 32, 32, False, "hook 8^2")
    check(got[:, 1280:].double().numpy(), hooks[1].numpy(), 32, 32, False, "hook 32^2")
    assert torch.equal(got[:, 1280:], feats["up-level3-repeat0-vit-block0-self-k"].cpu().contiguous())      # identity: the hook's bits


def test_cli_bilinear_aggregate(tmp_path, monkeypatch):
    monkeypatch.setenv("GDF_SYNTHETIC_WEIGHTS", "1")
    sys.path.insert(0, ROOT)
    import extract_feature as cli
    from test_gpu_cli import _setup
    layers = _setup(tmp_path)
    base = ["--layer", str(tmp_path / "layers.json"), "--version", "1-5", "--img_size", "256", "--t", "100", "-b", "2", "--seed", "3",
            "--input_dir", str(tmp_path / "imgs" / "*.png"), "--prompt_file", str(tmp_path / "prompt.txt"), "--use_original_filename"]
    cli.main(base + ["--output_dir", str(tmp_path / "plain")])
    cli.main(base + ["--output_dir", str(tmp_path / "agg"), "--aggregate_output", "--aggregate_mode", "bilinear", "--aggregate_size", "32"])
    assert sorted(os.listdir(tmp_path / "agg")) == ["a.npy", "b.npy", "c.npy"]
    for n in "abc":                                                              # (c: the ragged last batch)
        agg = np.load(tmp_path / "agg" / f"{n}.npy")
        assert agg.shape == (1600, 32, 32) and agg.dtype == np.float16
        off = 0
        for k in layers:
            v = np.load(tmp_path / "plain" / k / f"{n}.npy")
            check(agg[None, off:off + v.shape[0]].astype(np.float64), v[None].astype(np.float32), 32, 32, False, "%s %s" % (n, k))
            off += v.shape[0]
