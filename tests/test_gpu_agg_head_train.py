"""Trainable aggregation head on the GPU (-m gpu): the weight-gradient kernel of csrc/aggwgrad.hip through gdf_agghead_wgrad, the device repack
of csrc/agghead.hip through gdf_agghead_update / gdf_agghead_create_device (include/gdf_ops.h), and components/postproc.py
TrainableAggregationHead with FeatureExtractor.hyperfeature.

Kernel level: ONE gdf_agghead_wgrad call per case on a guard-filled dW (64 elements of tail) with a guard-tailed workspace.  The result is compared
with the float64 oracle of tests/agg_head_train_ref.py per input channel under a bound taken at run time from torch's own fp32 CPU weight gradient
on the same inputs (no fixed constant).  A workgroup of the kernel is 128 output channels x 32 input channels and walks over the pixels in 32 x 4
patches: the cases are sized around those numbers."""
import ctypes

import pytest
import torch

import agg_head_ref as AR
import agg_head_train_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, guard, is_guard

pytestmark = pytest.mark.gpu
TAIL = 64


def _lib():
    return R.bind(lib())


def wgrad(L, d, g, dw0=None, st=None):
    """d: the device map (any strides), g: the device gradient -> dW (Cout, Cin, 3, 3) fp32 on the CPU after the guard checks; dw0: accumulate onto it"""
    B, Cin, H, W = d.shape
    Cout = g.shape[1]
    n = Cout * Cin * 9
    out = guard((n + TAIL,), torch.float32)
    if dw0 is not None:
        out[:n] = dw0.cuda().reshape(-1)
    nbytes = L.gdf_agghead_wgrad_workspace(B, Cin, Cout, H, W)
    assert nbytes >= 8 * Cout
    ws = guard(((nbytes + 3) // 4 + TAIL,), torch.float32)
    src = R.agg_src(d.data_ptr(), d.dtype == torch.float32, d.stride(), d.shape)
    if st is not None:
        torch.cuda.synchronize()                                             # the guard fill runs on the current stream, the op on another
    ok(L.gdf_agghead_wgrad(ctypes.addressof(src), B, P(g), Cout, P(out), int(dw0 is not None), P(ws), nbytes,
                           st if st is not None else stream()), L)
    torch.cuda.synchronize()
    out, wsc = out.cpu(), ws.cpu()
    assert bool(is_guard(out[n:]).all()), "written behind dW"
    assert not bool(is_guard(out[:n]).any()), "owned elements of dW not written"
    assert bool(is_guard(wsc[(nbytes + 3) // 4:]).all()), "written behind the workspace"
    assert torch.equal(wsc[:Cout], g.abs().amax((0, 2, 3)).cpu())            # the pre-pass leaves max |G| per output channel
    return out[:n].view(Cout, Cin, 3, 3)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", list(R.CASES))
def test_one_call_against_the_oracle(name):
    x, g, bd = R.case(name)
    d = x.cuda()
    assert d.stride() == x.stride()
    bd.check(wgrad(_lib(), d, g.cuda()), name)


@pytest.mark.parametrize("where", ["corner", "edge", "interior", "seam", "last pixel of image 0"])
def test_planted_impulses_are_placed_as_the_gradient_places_them(where):
    """one element of G is 3; the map holds small distinct integers (exact in fp16): dW[co0, ci, dy, dx] = 3 X[b0, ci, y0 + dy - 1, x0 + dx - 1] bit
    for bit, exactly 0 where that tap lies in the padding, and exactly 0 in every other output channel"""
    Cin, Cout, B, H, W = 5, 4, 2, 6, 35
    b0, co0, y0, x0 = {"corner": (0, 0, 0, 0), "edge": (1, 2, 5, 17), "interior": (1, 1, 2, 3), "seam": (0, 3, 3, 31),
                       "last pixel of image 0": (0, 1, H - 1, W - 1)}[where]
    x = (1 + (torch.arange(B * Cin * H * W) * 37) % 509).view(B, Cin, H, W).float()
    g = torch.zeros(B, Cout, H, W)
    g[b0, co0, y0, x0] = 3.0
    want = torch.zeros(Cout, Cin, 3, 3)
    for dy in range(3):
        for dx in range(3):
            y, xx = y0 + dy - 1, x0 + dx - 1
            if 0 <= y < H and 0 <= xx < W:
                want[co0, :, dy, dx] = 3.0 * x[b0, :, y, xx]
    L = _lib()
    for dtype in (torch.float16, torch.float32):
        v = x.to(dtype)
        for d in (v.cuda(), _cl(v).cuda()):
            got = wgrad(L, d, g.cuda())
            assert same_bits(got, want), (where, dtype, d.stride(), (got - want).abs().max())


def test_zero_channel_accumulate_and_determinism():
    x, g, bd = R.case("C72 -> 36, B2 9x7")
    g = g.clone()
    g[:, 7] = 0
    L = _lib()
    d, gd = x.cuda(), g.cuda()
    first = wgrad(L, d, gd)
    R.Bounds(x, g).check(first, "an all-zero channel of G")
    assert float(first[7].abs().max()) == 0 and not bool(torch.signbit(first[7]).any())    # exactly 0
    again = wgrad(L, d, gd)
    s1 = torch.cuda.Stream()
    other = wgrad(L, d, gd, st=vp(s1.cuda_stream))
    assert same_bits(again, first) and same_bits(other, first)               # the same inputs: the same bits, on any stream
    dw0 = torch.randn(first.shape, generator=torch.Generator().manual_seed(3)) * float(first.abs().mean())
    assert same_bits(wgrad(L, d, gd, dw0=dw0), dw0 + first)                  # accumulate: the complete sum, added once


def test_strided_views_keep_the_nan_padding_out():
    """the map is a view into a larger NaN-filled buffer: x stride 2 inside an NCHW buffer, and a channels-last buffer whose pixels are 8 channels
    longer than C; the zero padding must come from the kernel, not from the NaNs that lie beside the map"""
    x, g, bd = R.case("C72 -> 36, B2 9x7")
    B, Cin, H, W = x.shape
    L = _lib()
    buf = torch.full((B, Cin + 3, H + 2, 2 * W + 1), float("nan"), dtype=x.dtype, device="cuda")
    view = buf[:, 1:Cin + 1, 1:H + 1, 1:2 * W:2]
    view.copy_(x)
    buf2 = torch.full((B, H + 1, W + 2, Cin + 8), float("nan"), dtype=x.dtype, device="cuda")
    view2 = buf2[:, :H, 1:W + 1, :Cin].permute(0, 3, 1, 2)
    view2.copy_(x)
    for what, d in (("x stride 2", view), ("padded channels-last pixels", view2)):
        assert tuple(d.shape) == tuple(x.shape) and not d.is_contiguous()
        got = wgrad(L, d, g.cuda())
        assert bool(torch.isfinite(got).all()), what
        bd.check(got, what)


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    d = R.gen_features(2, 8, 4, 4, False, 1415).cuda()
    g = R.gen_grad(2, 5, 4, 4, 1416).cuda()
    n = 5 * 8 * 9
    out = guard((n + TAIL,), torch.float32)
    nbytes = L.gdf_agghead_wgrad_workspace(2, 8, 5, 4, 4)
    ws = guard(((nbytes + 3) // 4,), torch.float32)
    src = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def call(B=2, s=src, gg=g, o=out, Cout=5, w=ws, nb=nbytes, acc=0):
        return L.gdf_agghead_wgrad(ctypes.addressof(s) if s is not None else None, B, P(gg), Cout, P(o), acc, P(w), nb, stream())
    assert call(s=None) == R.GDF_ERR_ARG and call(gg=None) == R.GDF_ERR_ARG and call(o=None) == R.GDF_ERR_ARG and call(w=None) == R.GDF_ERR_ARG
    assert b"gdf_agghead_wgrad" in L.gdf_last_error()
    assert call(B=-1) == R.GDF_ERR_ARG and call(Cout=0) == R.GDF_ERR_ARG and call(nb=nbytes - 1) == R.GDF_ERR_ARG
    for field in ("C", "H", "W"):
        keep = getattr(src, field)
        setattr(src, field, 0)
        assert call() == R.GDF_ERR_ARG, field
        setattr(src, field, keep)
    ptr, src.ptr = src.ptr, None
    assert call() == R.GDF_ERR_ARG
    src.ptr = ptr
    src.H, src.W = 1 << 16, 1 << 15                                          # B * H * W = 2^31 (refused before anything is read)
    assert call(B=1, nb=1 << 62) == R.GDF_ERR_ARG
    src.H, src.W = 4, 4
    assert call(B=0) == 0 and call(B=0, acc=1) == 0                          # a no-op: nothing is launched, dW is not zeroed
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all()) and bool(is_guard(ws.cpu()).all())
    assert call() == 0
    torch.cuda.synchronize()
    # the repack
    w, _ = R.gen_weight(5, 8, 1417)
    wd = w.cuda()
    o = vp()
    assert L.gdf_agghead_create_device(8, 5, None, None, stream(), ctypes.byref(o)) == R.GDF_ERR_ARG and not o.value
    assert L.gdf_agghead_create_device(8, 5, P(wd), None, stream(), None) == R.GDF_ERR_ARG
    assert L.gdf_agghead_create_device(0, 5, P(wd), None, stream(), ctypes.byref(o)) == R.GDF_ERR_ARG
    assert L.gdf_agghead_create_device(8, 0, P(wd), None, stream(), ctypes.byref(o)) == R.GDF_ERR_ARG
    assert b"gdf_agghead_create_device" in L.gdf_last_error()
    assert L.gdf_agghead_update(None, P(wd), stream()) == R.GDF_ERR_ARG
    h = vp()
    ok(L.gdf_agghead_create(8, 5, vp(w.data_ptr()), None, ctypes.byref(h)), L)
    try:
        assert L.gdf_agghead_update(h, None, stream()) == R.GDF_ERR_ARG
        assert b"gdf_agghead_update" in L.gdf_last_error()
    finally:
        L.gdf_agghead_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# repack
# ------------------------------------------------------------------------------------------------------------------------------
def forward(L, h, Cout, d):
    B, _, H, W = d.shape
    n = B * Cout * H * W
    out = guard((n + TAIL,), torch.float32)
    src = R.agg_src(d.data_ptr(), d.dtype == torch.float32, d.stride(), d.shape)
    ok(L.gdf_agghead_forward(h, ctypes.addressof(src), B, P(out), stream()), L)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(is_guard(out[n:]).all()) and not bool(is_guard(out[:n]).any())
    return out[:n].view(B, Cout, H, W)


def host_head(L, w, bias=None):
    h = vp()
    ok(L.gdf_agghead_create(w.shape[1], w.shape[0], vp(w.data_ptr()), vp(bias.data_ptr()) if bias is not None else None, ctypes.byref(h)), L)
    return h


def _extreme(w):
    w = w.clone()
    w[1] = 0                                                                 # an all-zero row
    w[2] *= 2.0 ** -120 / float(w[2].abs().max())                            # rows whose largest magnitudes are 2^-120 and 2^100
    w[3] *= 2.0 ** 100 / float(w[3].abs().max())
    return w.contiguous()


REPACK = {"8 -> 5": (8, 5, 0), "72 -> 36": (72, 36, 0), "200 -> 72": (200, 72, 0), "Cout 257": (24, 257, 0), "zero and extreme rows": (40, 9, 1)}


@pytest.mark.parametrize("name", list(REPACK))
def test_device_repack_gives_the_host_pack_bit_for_bit(name):
    Cin, Cout, extreme = REPACK[name]
    seed = sum(map(ord, name))
    w1, _ = R.gen_weight(Cout, Cin, seed)
    w2, b2 = R.gen_weight(Cout, Cin, seed + 1, bias=True)
    if extreme:
        w2 = _extreme(w2)
    d = R.gen_features(1, Cin, 5, 6, False, seed + 2).cuda()
    L = _lib()
    want_h = host_head(L, w2)
    upd_h = host_head(L, w1)
    dev_h, devb_h, wantb_h = vp(), vp(), host_head(L, w2, b2)
    try:
        want = forward(L, want_h, Cout, d)
        assert not same_bits(forward(L, upd_h, Cout, d), want)
        w2d, b2d = w2.cuda(), b2.cuda()
        ok(L.gdf_agghead_update(upd_h, P(w2d), stream()), L)
        assert same_bits(forward(L, upd_h, Cout, d), want), "update"
        ok(L.gdf_agghead_create_device(Cin, Cout, P(w2d), None, stream(), ctypes.byref(dev_h)), L)
        assert same_bits(forward(L, dev_h, Cout, d), want), "create_device"
        ok(L.gdf_agghead_create_device(Cin, Cout, P(w2d), P(b2d), stream(), ctypes.byref(devb_h)), L)
        assert same_bits(forward(L, devb_h, Cout, d), forward(L, wantb_h, Cout, d)), "create_device with a bias"
        w1d = w1.cuda()
        ok(L.gdf_agghead_update(devb_h, P(w1d), stream()), L)                # back again, on a device-created handle; the bias stays
        ok(L.gdf_agghead_update(wantb_h, P(w1d), stream()), L)
        back = forward(L, devb_h, Cout, d)
        assert same_bits(back, forward(L, wantb_h, Cout, d))
        if not extreme:
            AR.Bounds(w1, b2, d.cpu()).check(back, "updated head, " + name)
    finally:
        for h in (want_h, upd_h, dev_h, devb_h, wantb_h):
            L.gdf_agghead_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# module
# ------------------------------------------------------------------------------------------------------------------------------
def test_one_training_step_through_the_native_head():
    from components import postproc
    w, x1, x2, src, tgt = R.step_inputs()
    want, bound, ref_err = R.step_bounds()
    head = postproc.TrainableAggregationHead(w).cuda()
    a, b = head(x1.cuda()), head(x2.cuda())
    assert a.is_cuda and a.dtype == torch.float32 and a.requires_grad
    assert same_bits(a.detach().cpu(), postproc.AggregationHead(w)(x1.cuda()).cpu())
    loss = postproc.clip_loss(a, b, src, tgt)[0]
    loss.backward()
    grad = head.out.weight.grad
    assert grad.is_cuda and tuple(grad.shape) == (8, 8, 3, 3)
    err = R.channel_error(grad.cpu(), want)
    print("native training step: worst channel error %.3e, bound %.3e (reference fp32 chain: %.3e)" % (err, bound, ref_err))
    assert err <= bound


def _count_updates(postproc):
    L = postproc._L()
    real, calls = L.gdf_agghead_update, []

    def wrapper(*a):
        calls.append(1)
        return real(*a)
    L.gdf_agghead_update = wrapper
    return L, real, calls


def test_the_packed_weights_follow_the_parameter():
    from components import postproc
    w, x1, x2, src, tgt = R.step_inputs()
    d = x1.cuda()
    head = postproc.TrainableAggregationHead(w).cuda()
    opt = torch.optim.AdamW(head.parameters(), lr=5e-4, weight_decay=0.01)
    L, real, calls = _count_updates(postproc)
    try:
        loss = postproc.clip_loss(head(d), head(x2.cuda()), src, tgt)[0]
        loss.backward()
        assert not calls                                                     # created from the weights as they were: nothing to refresh
        opt.step()
        after = head(d).detach()
        assert len(calls) == 1
        assert same_bits(after.cpu(), postproc.AggregationHead(head.out.weight)(d).cpu())      # the refresh, proven
        assert not torch.equal(head.out.weight.detach().cpu(), w)
        with torch.no_grad():
            head(d), head(x2.cuda()), head.eval()(d), head.train()(d)
        assert len(calls) == 1                                               # nothing changed: no refresh
        w2, _ = R.gen_weight(8, 8, 99)
        head.load_state_dict({"out.weight": w2})
        assert same_bits(head(d).detach().cpu(), postproc.AggregationHead(w2)(d).cpu()) and len(calls) == 2
        with torch.no_grad():
            head.out.weight.copy_(w)
        assert same_bits(head(d).detach().cpu(), postproc.AggregationHead(w)(d).cpu()) and len(calls) == 3
        head.refresh()
        assert len(calls) == 4 and same_bits(head(d).detach().cpu(), postproc.AggregationHead(w)(d).cpu()) and len(calls) == 4
        back = head.cpu()                                                    # the module moves: the host path, then the device again
        assert torch.equal(back(x1).detach(), torch.nn.functional.conv2d(x1.float(), w, padding=1))
        assert same_bits(head.cuda()(d).detach().cpu(), postproc.AggregationHead(w)(d).cpu())
    finally:
        L.gdf_agghead_update = real


def test_twenty_steps_lower_the_loss():
    from components import postproc
    x1, x2, src, tgt = R.run_inputs()
    head = postproc.TrainableAggregationHead(R.run_head()).cuda()
    losses = R.training_run(head, lambda a, b, s, t: postproc.clip_loss(a, b, s, t)[0], x1.cuda(), x2.cuda(), src, tgt)
    print("native run: loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert len(losses) == R.RUN["steps"] + 1 and losses[-1] < losses[0]


def test_hyperfeature_and_the_value_errors():
    import diffusion_feature
    from components import postproc
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    w, _ = R.gen_weight(5, 12, 51)
    head = postproc.TrainableAggregationHead(w).cuda()
    feats = {"a": R.gen_features(2, 8, 10, 9, False, 52).cuda(), "b": R.gen_features(2, 4, 5, 5, False, 53).cuda()}
    got = fe.hyperfeature(head, feats, (10, 9))
    want = head(postproc.aggregate(list(feats.values()), (10, 9)))
    assert got.requires_grad and same_bits(got.detach().cpu(), want.detach().cpu())
    got.sum().backward()
    assert head.out.weight.grad is not None and head.out.weight.grad.is_cuda
    with pytest.raises(ValueError, match="gradient"):
        head(torch.zeros(1, 12, 4, 4, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="module"):
        postproc.TrainableAggregationHead(w)(torch.zeros(1, 12, 4, 4, device="cuda"))       # the module is still on the host
    with pytest.raises(ValueError):
        head(torch.zeros(1, 11, 4, 4, device="cuda"))
    assert tuple(head(torch.zeros(0, 12, 4, 4, device="cuda")).shape) == (0, 5, 4, 4)
