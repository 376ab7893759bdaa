"""Aggregation-network head on the GPU (-m gpu): the kernel of csrc/agghead.hip through gdf_agghead_* (include/gdf_ops.h), components/postproc.py
AggregationHead and FeatureExtractor.hyperfeature.

Kernel level: ONE gdf_agghead_forward call per case.  The output is compared with the float64 oracle of tests/agg_head_ref.py per block of 16
pixels under a bound taken at run time from the reference's own fp32 arithmetic on the same inputs (no fixed constant); it is guard-filled with 64
elements of tail as in tests/test_gpu_pixel_classifier.py.  A workgroup of the kernel is 256 output channels x a 32 x 4 pixel patch and stages 32
input channels at a time: the cases are sized around those numbers."""
import ctypes
import functools

import pytest
import torch

import agg_head_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, guard, is_guard

pytestmark = pytest.mark.gpu
TAIL = 64
ROWS, PW, PH = 256, 32, 4                                                    # a workgroup's output channels and pixel patch


def _lib():
    return R.bind(lib())


def create(L, w, bias=None):
    h = vp()
    ok(L.gdf_agghead_create(w.shape[1], w.shape[0], vp(w.data_ptr()), vp(bias.data_ptr()) if bias is not None else None, ctypes.byref(h)), L)
    return h


def launch(L, h, Cout, d, st=None):
    """d: the device map (any strides) -> (B, Cout, H, W) fp32 on the CPU after the guard checks"""
    B, _, H, W = d.shape
    n = B * Cout * H * W
    out = guard((n + TAIL,), torch.float32)
    src = R.agg_src(d.data_ptr(), d.dtype == torch.float32, d.stride(), d.shape)
    if st is not None:
        torch.cuda.synchronize()                                             # the guard fill runs on the current stream, the op on another
    ok(L.gdf_agghead_forward(h, ctypes.addressof(src), B, P(out), st if st is not None else stream()), L)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(is_guard(out[n:]).all()), "written behind the output"
    assert not bool(is_guard(out[:n]).any()), "owned outputs not written"
    return out[:n].view(B, Cout, H, W)


@functools.lru_cache(maxsize=None)
def case_data(Cin, Cout, B, H, W, f32, seed, bias=False):
    """inputs, oracle and bound of one case, computed once and shared (never modified)"""
    w, b = R.gen_weight(Cout, Cin, seed, bias)
    v = R.gen_features(B, Cin, H, W, bool(f32), seed + 1)
    return w, b, v, R.Bounds(w, b, v)


# name: (Cin, Cout, B, H, W, fp32 map, channels-last)
CASES = {
    "C8 -> 5, 6x6 fp16 NCHW": (8, 5, 1, 6, 6, 0, 0),                         # fewer channels than one k-step, one partial tile
    "C72 -> 36, B2 9x7": (72, 36, 2, 9, 7, 0, 0),                            # k-tile tail, partial 32-row block, odd width; image 1 follows image 0's last row
    "one row": (40, 7, 1, 1, 37, 0, 0),                                      # every vertical tap in the padding, two patches along x
    "one column": (40, 7, 1, 37, 1, 0, 1),                                   # every horizontal tap in the padding
    "one pixel": (40, 7, 2, 1, 1, 0, 0),
    "C200 -> 72, 17x16 channels-last": (200, 72, 2, 17, 16, 0, 1),           # several tiles, 16-byte loads stopping at C
    "C8 -> 5 fp32 NCHW": (8, 5, 1, 6, 6, 1, 0),                              # the three-pass path
    "C136 -> 40 fp32 channels-last": (136, 40, 2, 12, 12, 1, 1),
    "Cout one row over a workgroup's": (24, ROWS + 1, 1, 8, 9, 0, 0),        # more than one Cout tile, a one-row tail
    "one pixel over a patch each way": (16, 8, 1, PH + 1, PW + 1, 0, 0),     # every tap crosses a tile seam
    "C3520 -> 40, 6x5": (3520, 40, 1, 6, 5, 0, 0),                           # the reference's depths: 110 and 230 channel tiles
    "C7360 -> 40, 6x5": (7360, 40, 1, 6, 5, 0, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_against_the_oracle(name):
    Cin, Cout, B, H, W, f32, chlast = CASES[name]
    w, _, v, bd = case_data(Cin, Cout, B, H, W, f32, sum(map(ord, name)))
    L = _lib()
    h = create(L, w)
    try:
        d = (_cl(v) if chlast else v).cuda()
        assert d.stride() == (_cl(v) if chlast else v).stride()
        bd.check(launch(L, h, Cout, d), name)
    finally:
        L.gdf_agghead_destroy(h)


def test_bias_and_an_all_zero_row():
    Cin, Cout, B, H, W = 40, 9, 1, 5, 6
    w, b, v, _ = case_data(Cin, Cout, B, H, W, 0, 2020, True)
    w = w.clone()
    w[4] = 0
    bd = R.Bounds(w, b, v)
    L = _lib()
    h = create(L, w, b)
    try:
        got = launch(L, h, Cout, v.cuda())
    finally:
        L.gdf_agghead_destroy(h)
    bd.check(got, "bias")
    assert torch.equal(got[:, 4], b[4].expand(B, H, W))                      # an all-zero row yields its bias


@pytest.mark.parametrize("where", ["corner", "edge", "interior", "seam"])
def test_planted_impulses_are_placed_as_cross_correlation_places_them(where):
    """one input element is 1.0; the weights are small distinct integers (exact in fp16, asymmetric under flips and transposes): the output equals,
    bit for bit, out[co, y0 - dy + 1, x0 - dx + 1] = W[co, ci0, dy, dx]"""
    Cin, Cout, H, W = 3, 4, 6, 35
    ci0, y0, x0 = {"corner": (0, 0, 0), "edge": (2, 5, 17), "interior": (1, 2, 3), "seam": (1, 3, 31)}[where]
    w = (torch.arange(Cout * Cin * 9, dtype=torch.float32) + 1).view(Cout, Cin, 3, 3)
    want = torch.zeros(1, Cout, H, W)
    for dy in range(3):
        for dx in range(3):
            y, x = y0 - dy + 1, x0 - dx + 1
            if 0 <= y < H and 0 <= x < W:
                want[0, :, y, x] = w[:, ci0, dy, dx]
    L = _lib()
    h = create(L, w)
    try:
        for dtype in (torch.float16, torch.float32):
            v = torch.zeros(1, Cin, H, W, dtype=dtype)
            v[0, ci0, y0, x0] = 1.0
            for d in (v.cuda(), _cl(v).cuda()):
                got = launch(L, h, Cout, d)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (where, dtype, d.stride())
    finally:
        L.gdf_agghead_destroy(h)


def test_strided_views_keep_the_nan_padding_out():
    """the map is a view into a larger NaN-filled buffer: x stride 2 inside an NCHW buffer (the any-stride path), and a channels-last buffer whose
    pixels are 8 channels longer than C (16-byte loads along C must stop at C); the conv's zero padding must come from the kernel, not from the
    NaNs that lie beside the map"""
    Cin, Cout, B, H, W = 72, 36, 2, 6, 5
    w, _, v, bd = case_data(Cin, Cout, B, H, W, 0, 1111)
    L = _lib()
    h = create(L, w)

    def nchw_view():
        buf = torch.full((B, Cin + 3, H + 2, 2 * W + 1), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, 1:Cin + 1, 1:H + 1, 1:2 * W:2]
        view.copy_(v)
        return buf, view

    def cl_view():
        buf = torch.full((B, H + 1, W + 2, Cin + 8), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, :H, 1:W + 1, :Cin].permute(0, 3, 1, 2)
        view.copy_(v)
        return buf, view

    try:
        for what, mk in (("x stride 2", nchw_view), ("padded channels-last pixels", cl_view)):
            buf, d = mk()
            assert tuple(d.shape) == (B, Cin, H, W) and not d.is_contiguous() and bool(torch.isnan(buf).any())
            got = launch(L, h, Cout, d)
            assert bool(torch.isfinite(got).all()), what
            bd.check(got, what)
    finally:
        L.gdf_agghead_destroy(h)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_streams_batches_and_determinism():
    Cin, Cout, B, H, W = 72, 40, 3, 9, 35
    w, _, v, bd = case_data(Cin, Cout, B, H, W, 0, 1212)
    L = _lib()
    h = create(L, w)
    try:
        d = v.cuda()
        first = launch(L, h, Cout, d)
        again = launch(L, h, Cout, d)
        s1 = torch.cuda.Stream(priority=-1)                                  # (its own pool: the streams later tests draw are those they drew before)
        other = launch(L, h, Cout, d, st=vp(s1.cuda_stream))
        assert same_bits(again, first) and same_bits(other, first)           # the same inputs: the same bits, on any stream
        bd.check(first, "B = 3 NCHW")
        for b in range(B):                                                   # an image's bits depend neither on B nor on its place in the batch
            assert same_bits(launch(L, h, Cout, d[b:b + 1]), first[b:b + 1]), b
        bd.check(launch(L, h, Cout, _cl(d)), "channels-last copy")           # accepted too; equality between the two layouts is not required
    finally:
        L.gdf_agghead_destroy(h)


def test_python_wrappers_agree_with_the_c_call():
    import diffusion_feature
    from components.postproc import AggregationHead, aggregate, nn_match
    Cin, Cout, B, H, W = 72, 36, 2, 9, 7
    w, _, v, bd = case_data(Cin, Cout, B, H, W, 0, sum(map(ord, "C72 -> 36, B2 9x7")))
    L = _lib()
    h = create(L, w)
    try:
        d = _cl(v).cuda()
        want = launch(L, h, Cout, d)
        want32 = launch(L, h, Cout, d.float())
    finally:
        L.gdf_agghead_destroy(h)
    for name, src in R.sources(w).items():
        head = AggregationHead(src)
        got = head(d)
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and same_bits(got.cpu(), want), name
    assert same_bits(head(d.float()).cpu(), want32)
    one = head(d[1])                                                         # the reference's unbatched (Cin, H, W)
    assert tuple(one.shape) == (Cout, H, W) and same_bits(one.cpu(), want[1])
    assert tuple(head(d[:0]).shape) == (0, Cout, H, W)
    wb, bb = R.gen_weight(Cout, Cin, 77, bias=True)                          # a convolution with a bias is accepted as it is
    hb = AggregationHead(R.Network(wb, bb).out)
    R.Bounds(wb, bb, v).check(hb(d).cpu(), "wrapper with a bias")
    # FeatureExtractor.hyperfeature = aggregate, then the head
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    feats = {"a": d[:, :40], "b": torch.nn.functional.avg_pool2d(d[:, 40:].float(), 2, ceil_mode=True).half()}
    agg = aggregate(list(feats.values()), (12, 10))
    none = fe.hyperfeature(None, feats, (12, 10))
    assert none.dtype == torch.float16 and torch.equal(none, agg)            # do_conv=False
    hyper = fe.hyperfeature(head, feats, (12, 10))
    assert tuple(hyper.shape) == (B, Cout, 12, 10) and same_bits(hyper.cpu(), head(agg).cpu())
    assert same_bits(fe.hyperfeature(R.Network(w), feats, (12, 10)).cpu(), hyper.cpu())     # anything a head is built from
    R.Bounds(w, None, agg.cpu()).check(hyper.cpu(), "hyperfeature")
    # ... and feeds correspond unchanged: the same points as the host chain on the same tensors
    feats2 = {k: torch.flip(t, dims=(0, 3)) * 0.5 + t.roll(1, 2) for k, t in feats.items()}
    hyper2 = fe.hyperfeature(head, feats2, (12, 10))
    pts = torch.tensor([[[3.0, 4.0], [20.2, 7.7], [0.0, 0.0], [30.0, 24.0], [11.5, 18.5]]]).expand(B, -1, -1)
    p_dev, _ = fe.correspond(hyper, hyper2, pts, (31, 25))
    p_host, _ = nn_match(hyper.cpu(), hyper2.cpu(), pts, (31, 25))
    assert p_dev.is_cuda and torch.equal(p_dev.cpu(), p_host)


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    w, _ = R.gen_weight(5, 8, 1414)
    h = create(L, w)
    d = R.gen_features(2, 8, 4, 4, False, 1415).cuda()
    out = guard((2 * 5 * 16 + TAIL,), torch.float32)
    src = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def call(handle=h, B=2, o=out, s=src):
        return L.gdf_agghead_forward(handle, ctypes.addressof(s) if s is not None else None, B, P(o), stream())
    try:
        assert call(handle=None) == R.GDF_ERR_ARG and call(o=None) == R.GDF_ERR_ARG and call(s=None) == R.GDF_ERR_ARG
        assert call(B=-1) == R.GDF_ERR_ARG
        assert b"gdf_agghead_forward" in L.gdf_last_error()
        src.C = 9
        assert call() == R.GDF_ERR_ARG                                       # the wrong C
        src.C = 8
        src.H = 0
        assert call() == R.GDF_ERR_ARG
        src.H = 4
        ptr, src.ptr = src.ptr, None
        assert call() == R.GDF_ERR_ARG
        src.ptr = ptr
        src.H, src.W = 1 << 16, 1 << 15                                      # B * H * W = 2^31 (refused before anything is read)
        assert call(B=1) == R.GDF_ERR_ARG
        src.H, src.W = 4, 4
        assert call(B=0) == 0
        torch.cuda.synchronize()
        assert bool(is_guard(out.cpu()).all())
        # creation: nonsense is an argument error and no handle comes back
        o = vp()
        assert L.gdf_agghead_create(8, 5, None, None, ctypes.byref(o)) == R.GDF_ERR_ARG and not o.value
        assert L.gdf_agghead_create(0, 5, vp(w.data_ptr()), None, ctypes.byref(o)) == R.GDF_ERR_ARG
        assert L.gdf_agghead_create(8, 0, vp(w.data_ptr()), None, ctypes.byref(o)) == R.GDF_ERR_ARG
        assert L.gdf_agghead_create(8, 5, vp(w.data_ptr()), None, None) == R.GDF_ERR_ARG
        for bad in (float("nan"), float("inf")):
            wn = w.clone()
            wn[3, 2, 1, 1] = bad
            assert L.gdf_agghead_create(8, 5, vp(wn.data_ptr()), None, ctypes.byref(o)) == R.GDF_ERR_ARG and not o.value
        assert b"gdf_agghead_create" in L.gdf_last_error()
        L.gdf_agghead_destroy(None)
        assert call() == 0                                                   # the handle still works
        torch.cuda.synchronize()
    finally:
        L.gdf_agghead_destroy(h)
