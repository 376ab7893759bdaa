"""The correspondence loss on the GPU (-m gpu): the kernels of csrc/cliploss.hip through gdf_op_clip_loss / gdf_op_clip_loss_backward
(include/gdf_ops.h), components/postproc.py clip_loss / compute_clip_loss and FeatureExtractor.correspondence_loss.

Kernel level: ONE forward + backward per case against the float64 oracle of tests/clip_loss_ref.py, with the bounds that file derives from the
reference's own fp32 arithmetic on the same inputs (MARGIN x its error; the derived floor for the terms and the loss); no measured figure.  Every
output is guard-filled and the workspace guard-tailed as in tests/test_gpu_correspond.py: the owned elements written, everything behind them and
behind the reported workspace size untouched."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import clip_loss_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, bits, gen, guard, is_guard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT8, TAIL = 0xA5, 4096


def _lib():
    return R.bind(lib())


class Run:
    """one forward (and backward) on device tensors, guard checks included; results on the CPU"""

    def __init__(self, L, d1, d2, src, tgt, scale=R.SCALE, st=None, terms=True):
        self.L, self.d1, self.d2, self.src, self.tgt, self.scale = L, d1, d2, src, tgt, scale
        self.st = st if st is not None else stream()
        B, N = src.shape
        self.B, self.N = B, N
        assert src.is_contiguous() and tgt.is_contiguous() and src.dtype == torch.int64 and tgt.dtype == torch.int64 and src.is_cuda
        loss, tm = guard((B + 64,), torch.float32), guard((B * 2 * N + 64,), torch.float32)
        self.nbytes = L.gdf_op_clip_loss_workspace(B, N, d1.shape[1], d1.shape[2] * d1.shape[3], d2.shape[2] * d2.shape[3])
        self.ws = torch.full((self.nbytes + TAIL,), PAT8, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 16 == 0
        self.s1 = R.agg_src(d1.data_ptr(), d1.dtype == torch.float32, d1.stride(), d1.shape)
        self.s2 = R.agg_src(d2.data_ptr(), d2.dtype == torch.float32, d2.stride(), d2.shape)
        torch.cuda.current_stream().synchronize()                            # the guard fills are done before another stream writes
        ok(L.gdf_op_clip_loss(ctypes.addressof(self.s1), ctypes.addressof(self.s2), B, P(src), P(tgt), N, scale, P(loss), P(tm) if terms else None,
                              P(self.ws), self.nbytes, self.st), L)
        torch.cuda.synchronize()
        loss, tm = loss.cpu(), tm.cpu()
        assert bool(is_guard(loss[B:]).all()) and bool(is_guard(tm[B * 2 * N:]).all()), "written behind the outputs"
        assert not bool(is_guard(loss[:B]).any()), "loss not written"
        assert bool(is_guard(tm).all()) != terms, "terms"
        self._tail()
        self.loss, self.terms = loss[:B], tm[:B * 2 * N].view(B, 2, N)

    def _tail(self):
        assert bool((self.ws[self.nbytes:].cpu() == PAT8).all()), "written behind the reported workspace size"

    def backward(self, g=None, want=(True, True), st=None):
        """-> (grad_f1, grad_f2) on the CPU, None where not wanted"""
        g = torch.ones(self.B, device="cuda") if g is None else g
        outs = [guard((v.numel() + 64,), torch.float32) if w else None for v, w in zip((self.d1, self.d2), want)]
        torch.cuda.current_stream().synchronize()
        ok(self.L.gdf_op_clip_loss_backward(ctypes.addressof(self.s1), ctypes.addressof(self.s2), self.B, P(self.src), P(self.tgt), self.N, self.scale,
                                            P(g), P(outs[0]), P(outs[1]), P(self.ws), self.nbytes, st if st is not None else self.st), self.L)
        torch.cuda.synchronize()
        self._tail()
        res = []
        for o, v in zip(outs, (self.d1, self.d2)):
            if o is None:
                res.append(None)
                continue
            o = o.cpu()
            assert bool(is_guard(o[v.numel():]).all()), "written behind a gradient"
            assert not bool(is_guard(o[:v.numel()]).any()), "gradient elements not written"
            res.append(o[:v.numel()].view(v.shape))
        return res


def run(f1, f2, src, tgt, bd, what, scale=R.SCALE):
    """host tensors (their strides are kept on the device) -> one forward + backward, checked against the oracle"""
    d1, d2 = f1.cuda(), f2.cuda()
    assert d1.stride() == f1.stride() and d2.stride() == f2.stride()
    r = Run(_lib(), d1, d2, src.cuda(), tgt.cuda(), scale)
    g1, g2 = r.backward()
    bd.check(r.loss, r.terms, g1, g2, what=what)
    return r, g1, g2


def same(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_forward_and_backward_against_the_oracle(name):
    f1, f2, src, tgt, bd = R.case(name)
    run(f1, f2, src, tgt, bd, name)


def test_planted_identical_maps_with_scale_100():
    """f2 = f1, tgt = src, distinct pixels, z up to 100: finite, within bound, and the loss below the uniform value ln P"""
    f = R.features(1, 40, 6, 6, seed=5)
    idx = R.indices(1, 12, 36, 5, distinct=True)
    bd = R.Bounds(f, f, idx, idx, scale=100.0)
    r, g1, g2 = run(f, f.clone(), idx, idx, bd, "planted, scale 100", scale=100.0)
    assert bool(torch.isfinite(r.loss).all()) and bool(torch.isfinite(r.terms).all()) and float(r.loss) < math.log(36)
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())


def test_a_null_gradient_leaves_the_other_unchanged_and_grad_loss_is_linear():
    f1, f2, src, tgt, bd = R.case("C 72 channels-last B 2 N 64")
    r = Run(_lib(), f1.cuda(), f2.cuda(), src.cuda(), tgt.cuda())
    g = torch.tensor([0.75, -1.5], device="cuda")
    g1, g2 = r.backward(g)
    only1, none2 = r.backward(g, want=(True, False))
    none1, only2 = r.backward(g, want=(False, True))
    assert none1 is None and none2 is None and same(only1, g1) and same(only2, g2)
    d1, d2 = r.backward(2 * g)                                               # x 2 is exact in fp32: exactly doubled bits
    assert same(d1, 2 * g1) and same(d2, 2 * g2)
    R.Bounds(f1, f2, src, tgt, g=g.cpu()).check(None, None, g1, g2, what="grad_loss (0.75, -1.5)")


def test_strided_views_keep_the_nan_padding_out():
    """both maps are views into larger NaN-filled buffers: x stride 2 inside an NCHW buffer (the any-stride path), and a channels-last buffer
    whose pixels are 8 channels longer than C (lanes along C must stop at C)"""
    B, C_, h, w, N = 2, 24, 6, 5, 16
    v1, v2 = R.features(B, C_, h, w, seed=31), R.features(B, C_, h, w, seed=32)
    src, tgt = R.indices(B, N, h * w, 33), R.indices(B, N, h * w, 34)
    bd = R.Bounds(v1, v2, src, tgt)

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
        r = Run(_lib(), d1, d2, src.cuda(), tgt.cuda())
        g1, g2 = r.backward()
        bd.check(r.loss, r.terms, g1, g2, what=what)


def test_streams_batch_positions_and_determinism():
    B, C_, N = 3, 48, 30
    f1, f2 = R.features(B, C_, 7, 7, seed=41), R.features(B, C_, 9, 8, seed=42)
    src, tgt = R.indices(B, N, 49, 43), R.indices(B, N, 72, 44)
    L = _lib()
    d1, d2, ds, dt = f1.cuda(), f2.cuda(), src.cuda(), tgt.cuda()

    def both(a, b, s, t, st=None):
        r = Run(L, a, b, s, t, st=st)
        return (r.loss, r.terms) + tuple(r.backward())

    first = both(d1, d2, ds, dt)
    again = both(d1, d2, ds, dt)
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    other = both(d1, d2, ds, dt, st=vp(s1.cuda_stream))
    for got in (again, other):                                               # the same inputs: the same bits, on any stream
        assert all(same(x, y) for x, y in zip(got, first))
    for b in range(B):                                                       # pair b of the B = 3 call against the B = 1 call
        one = both(d1[b:b + 1], d2[b:b + 1], ds[b:b + 1].contiguous(), dt[b:b + 1].contiguous())
        assert all(same(x, y[b:b + 1]) for x, y in zip(one, first)), b
    cl = both(_cl(d1), _cl(d2), ds, dt)                                      # accepted too; equality between the layouts is not required
    R.Bounds(f1, f2, src, tgt).check(*cl, what="channels-last copy")


def test_beside_a_gemm_on_a_second_stream_keeps_its_bits():
    """one forward + backward while a GEMM runs on a second stream: the bits equal the solo run.  Once, no loop."""
    B, C_, N = 2, 320, 20
    L = _lib()
    d1, d2 = R.features(B, C_, 16, 16, seed=61).cuda(), R.features(B, C_, 16, 16, seed=62).cuda()
    ds, dt = R.indices(B, N, 256, 63).cuda(), R.indices(B, N, 256, 64).cuda()
    r = Run(L, d1, d2, ds, dt)
    solo = (r.loss, r.terms) + tuple(r.backward())
    M = K = 4096
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    Wt = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    o16 = torch.zeros(M, M, dtype=torch.half, device="cuda")
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(6):                                                       # a few milliseconds of GEMM queued on s1, then the op on s0
        ok(L.gdf_op_gemm(P(A), K, P(Wt), None, None, None, 0, P(o16), M, None, 0, M, M, K, 0, vp(s1.cuda_stream)), L)
    r = Run(L, d1, d2, ds, dt, st=vp(s0.cuda_stream))
    beside = (r.loss, r.terms) + tuple(r.backward())
    assert all(same(x, y) for x, y in zip(beside, solo))
    assert bool(torch.isfinite(o16.float()).all())


def test_a_zeroed_pixel_makes_its_pair_nan_and_no_other():
    f1, f2, src, tgt, _ = R.case("C 72 channels-last B 2 N 64")
    f2 = f2.clone()
    f2[0, :, 2, 3] = 0                                                       # not a query or a label of pair 1; the reference's 0 / 0
    r = Run(_lib(), f1.cuda(), f2.cuda(), src.cuda(), tgt.cuda())
    g1, g2 = r.backward()
    assert math.isnan(float(r.loss[0])) and bool(torch.isnan(r.terms[0]).all())
    assert bool(torch.isnan(g1[0]).all()) and bool(torch.isnan(g2[0]).all())
    R.Bounds(f1[1:], f2[1:], src[1:], tgt[1:]).check(r.loss[1:], r.terms[1:], g1[1:], g2[1:], what="pair 1 beside a NaN pair")


def test_an_index_outside_its_map_gives_nan_and_touches_nothing_else():
    f1, f2, src, tgt, _ = R.case("two grids two types")
    for which, value in ((0, 81), (1, -1), (1, 1 << 40)):
        s, t = src.clone(), tgt.clone()
        (s, t)[which][1, 3] = value
        r = Run(_lib(), f1.cuda(), f2.cuda(), s.cuda(), t.cuda())            # the guards behind every output are checked inside
        g1, g2 = r.backward()
        assert math.isnan(float(r.loss[1])) and bool(torch.isnan(g1[1]).all()) and bool(torch.isnan(g2[1]).all())
        R.Bounds(f1[:1], f2[:1], src[:1], tgt[:1]).check(r.loss[:1], r.terms[:1], g1[:1], g2[:1], what="pair 0 beside an index out of range")


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    d = R.features(2, 8, 4, 4).cuda()
    idx = R.indices(2, 3, 16, 1).cuda()
    loss, g1, g2 = guard((2,), torch.float32), guard((256,), torch.float32), guard((256,), torch.float32)
    nbytes = L.gdf_op_clip_loss_workspace(2, 3, 8, 16, 16)
    ws = torch.full((nbytes,), PAT8, dtype=torch.uint8, device="cuda")
    s1, s2 = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape), R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def fwd(B=2, N=3, scale=14.0, nb=nbytes):
        return L.gdf_op_clip_loss(ctypes.addressof(s1), ctypes.addressof(s2), B, P(idx), P(idx), N, scale, P(loss), None, P(ws), nb, stream())

    def bwd(B=2, N=3, scale=14.0, nb=nbytes):
        return L.gdf_op_clip_loss_backward(ctypes.addressof(s1), ctypes.addressof(s2), B, P(idx), P(idx), N, scale, P(loss), P(g1), P(g2), P(ws), nb,
                                           stream())
    for call, name in ((fwd, b"gdf_op_clip_loss"), (bwd, b"gdf_op_clip_loss_backward")):
        assert call(N=0) == R.GDF_ERR_ARG and call(scale=0.0) == R.GDF_ERR_ARG and call(nb=nbytes - 1) == R.GDF_ERR_ARG and call(B=-1) == R.GDF_ERR_ARG
        assert name in L.gdf_last_error()
        s2.C = 9
        assert call() == R.GDF_ERR_ARG
        s2.C = 8
        assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(bool(is_guard(t.cpu()).all()) for t in (loss, g1, g2)) and bool((ws.cpu() == PAT8).all())


# ------------------------------------------------------------------------------------------------------------------------------
# Python level
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers_agree_with_the_c_calls():
    import diffusion_feature
    from components.postproc import clip_loss, compute_clip_loss
    f1, f2, src, tgt, bd = R.case("two grids two types")                     # fp32 NCHW against fp16 channels-last
    d1, d2 = f1.cuda().requires_grad_(True), f2.cuda().requires_grad_(True)
    r = Run(_lib(), d1.detach(), d2.detach(), src.cuda(), tgt.cuda())
    w1, w2 = r.backward()
    loss = clip_loss(d1, d2, src, tgt)                                       # host indices are moved; the result stays on the device
    assert loss.is_cuda and loss.dtype == torch.float32 and tuple(loss.shape) == (2,)
    loss.sum().backward()
    assert same(loss.detach().cpu(), r.loss)
    assert d1.grad.dtype == torch.float32 and d2.grad.dtype == torch.float16 and d1.grad.shape == d1.shape and d2.grad.shape == d2.shape
    assert same(d1.grad.cpu(), w1) and same(d2.grad.cpu(), w2.half())
    # a gradient only for the input that requires one
    e1 = f1.cuda().requires_grad_(True)
    clip_loss(e1, d2.detach(), src, tgt).sum().backward()
    assert same(e1.grad.cpu(), w1)
    # FeatureExtractor.correspondence_loss from points, compute_clip_loss on one pair
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    p1 = torch.stack([src // 9, src % 9], -1).double() + 0.25
    p2 = torch.stack([tgt // 12, tgt % 12], -1).double() - 0.25
    assert same(fe.correspondence_loss(d1.detach(), d2.detach(), p1, p2).cpu(), r.loss)
    sq1, sq2, ssrc, stgt, _ = R.case("C 40 on 6 x 6")
    one = Run(_lib(), sq1.cuda(), sq2.cuda(), ssrc.cuda(), stgt.cuda())
    pts = lambda i: np.stack([(i // 6).numpy(), (i % 6).numpy()], -1).astype(np.float64)  # noqa: E731
    got = compute_clip_loss(None, sq1.cuda(), sq2.cuda(), pts(ssrc[0]), pts(stgt[0]), (6, 6))
    assert got.dim() == 0 and got.is_cuda and same(got.cpu()[None], one.loss)


def test_a_training_step_through_a_torch_convolution():
    """torch conv -> device loss -> backward: weight.grad within MARGIN x the fp32 CPU chain's error against the float64 chain"""
    from components.postproc import clip_loss
    g = gen(71)
    conv = torch.nn.Conv2d(8, 8, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(8, 8, 3, 3, generator=g) / 8)
    x1, x2 = torch.randn(1, 8, 6, 6, generator=g), torch.randn(1, 8, 6, 6, generator=g)
    src, tgt = R.indices(1, 12, 36, 72), R.indices(1, 12, 36, 73)

    def step(dtype, device, loss_fn):
        c = torch.nn.Conv2d(8, 8, 3, padding=1, bias=False).to(dtype)
        with torch.no_grad():
            c.weight.copy_(conv.weight.to(dtype))
        c = c.to(device)
        loss = loss_fn(c(x1.to(device, dtype)), c(x2.to(device, dtype)))
        loss.backward()
        return c.weight.grad.detach().cpu().double()

    def chain(full):
        def fn(a, b):
            return R._chain_loss(a, b, src, tgt, R.SCALE, full)
        return fn
    want = step(torch.float64, "cpu", chain(False))
    ref = step(torch.float32, "cpu", chain(True))
    got = step(torch.float32, "cuda", lambda a, b: clip_loss(a, b, src, tgt).sum())
    ref_err, err = float((ref - want).norm() / want.norm()), float((got - want).norm() / want.norm())
    print("training step: weight.grad error %.3e, bound %.3e (reference fp32: %.3e)" % (err, R.MARGIN * ref_err, ref_err))
    assert math.isfinite(err) and err <= R.MARGIN * ref_err


@pytest.mark.parametrize("name", ["c40_6x6", "smoothed_9x9", "f32_8x8"])
def test_reference_results_on_the_device(name):
    from components.postproc import compute_clip_loss, points_to_idxs
    z = np.load(os.path.join(ROOT, "tests", "golden", "clip_loss.npz"))
    f1, f2 = torch.from_numpy(z[name + ":f1"]), torch.from_numpy(z[name + ":f2"])
    sp, tp, size = z[name + ":source_points"], z[name + ":target_points"], tuple(int(v) for v in z[name + ":output_size"])
    d1, d2 = f1.cuda().requires_grad_(True), f2.cuda().requires_grad_(True)
    loss = compute_clip_loss(None, d1, d2, sp, tp, size)
    loss.backward()
    src = torch.from_numpy(points_to_idxs(sp, size).astype(np.int64))[None]
    tgt = torch.from_numpy(points_to_idxs(tp, size).astype(np.int64))[None]
    bd = R.Bounds(f1, f2, src, tgt)
    if d1.dtype == torch.float32:
        bd.check(loss.detach().cpu()[None], None, d1.grad.cpu(), d2.grad.cpu(), what="golden on the device, " + name)
    else:
        # fp16 maps get fp16 gradients.  The loss against the oracle; a gradient against the reference's: rounding x to fp16 errs by at most
        # max(2^-11 |x|, 2^-25) (the second for subnormals), so the relative L2 error is at most sqrt(2^-22 + n 2^-50 / ||ref||^2), plus the fp32
        # bound of the value that was rounded and the reference's own error
        bd.check(loss.detach().cpu()[None], None, None, None, what="golden on the device, " + name)
        for got, key, b, r in ((d1.grad, "grad_f1", bd.b_g1, bd.ref_g1), (d2.grad, "grad_f2", bd.b_g2, bd.ref_g2)):
            ref = torch.from_numpy(z[name + ":" + key]).double()
            err = float((got.cpu().double() - ref).norm() / ref.norm())
            bound = math.sqrt(2.0 ** -22 + ref.numel() * 2.0 ** -50 / float(ref.norm()) ** 2) + b + r
            print("clip loss golden on the device, %s: fp16 %s error %.3e, bound %.3e" % (name, key, err, bound))
            assert got.dtype == torch.float16 and err <= bound
    assert abs(float(loss.detach()) - float(z[name + ":loss"])) <= bd.b_loss + bd.ref_loss
