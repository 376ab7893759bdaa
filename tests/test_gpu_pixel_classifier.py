"""Pixel-classifier ensemble on the GPU (-m gpu): the kernels of csrc/pixcls.hip through gdf_pixcls_* (include/gdf_ops.h), components/postproc.py
PixelClassifierEnsemble / predict_labels and FeatureExtractor.segment.

Kernel level: ONE gdf_pixcls_predict call per case.  The logits are compared with the float64 oracle of tests/pixel_classifier_ref.py per block of
16 pixels under a bound taken at run time from the reference's own fp32 arithmetic on the same inputs (no fixed constant); the decisions (per-model
labels, final label, js, top_k) are checked as exact functions of the DEVICE's own logits; the final labels against the oracle's off ambiguous
pixels.  Outputs and the workspace are guard-filled as in tests/test_gpu_correspond.py."""
import ctypes
import functools

import pytest
import torch

import pixel_classifier_ref as R
from ops_binding import P, lib, ok, stream, vp
from test_gpu_glue import _cl, guard, is_guard

pytestmark = pytest.mark.gpu
PAT64, PAT8, TAIL = 0x7FDA7FDA7FDA7FDA, 0xA5, 4096


def _lib():
    return R.bind(lib())


def create(L, sds):
    """state dicts -> (handle, the Python-side ensemble whose folded parameters it was made from)"""
    from components.postproc import PixelClassifierEnsemble
    ens = PixelClassifierEnsemble(sds)
    h = vp()
    ok(L.gdf_pixcls_create(ens.C, ens.M, ens.h1, ens.h2, ens.K, *[vp(t.data_ptr()) for t in ens.folded], ctypes.byref(h)), L)
    return h, ens


def launch(L, h, M, K, d, st=None, outs=True):
    """d: the device map (any strides) -> (labels (P,), js (P,), model labels (M, P), logits (M, P, K)) on the CPU after the guard checks;
    outs = False: the optional outputs are NULL and the logits stay in the workspace (-> labels only)"""
    B, _, H, W = d.shape
    n = B * H * W
    labels = torch.full((n + 64,), PAT64, dtype=torch.int64, device="cuda")
    js, logits = guard((n + 64,), torch.float32), guard((M * n * K + 64,), torch.float32)
    mlab = torch.full((M * n + 64,), PAT8, dtype=torch.uint8, device="cuda")
    nbytes = L.gdf_pixcls_workspace(h, B, H, W)
    ws = torch.full((nbytes + TAIL,), PAT8, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and nbytes >= M * n * K * 4
    src = R.agg_src(d.data_ptr(), d.dtype == torch.float32, d.stride(), d.shape)
    ok(L.gdf_pixcls_predict(h, ctypes.addressof(src), B, P(labels), P(js) if outs else None, P(mlab) if outs else None,
                            P(logits) if outs else None, P(ws), nbytes, st if st is not None else stream()), L)
    torch.cuda.synchronize()
    labels, js, mlab, logits, ws = labels.cpu(), js.cpu(), mlab.cpu(), logits.cpu(), ws.cpu()
    assert bool((labels[n:] == PAT64).all()) and bool(is_guard(js[n:]).all()) and bool((mlab[M * n:] == PAT8).all()), "written behind the outputs"
    assert bool(is_guard(logits[M * n * K:]).all()) and bool((ws[nbytes:] == PAT8).all()), "written behind the logits or the workspace"
    assert not bool((labels[:n] == PAT64).any()), "labels not written"
    if not outs:
        assert bool(is_guard(js).all()) and bool((mlab == PAT8).all()) and bool(is_guard(logits).all())
        return labels[:n]
    assert not bool(is_guard(js[:n]).any()) and not bool(is_guard(logits[:M * n * K]).any()), "owned outputs not written"
    return labels[:n], js[:n], mlab[:M * n].view(M, n), logits[:M * n * K].view(M, n, K)


def check(got, bd, M, K, B, what):
    """one call's outputs against the oracle and against the device's own logits"""
    labels, js, mlab, logits = got
    bd.check_logits(logits, what)
    assert torch.equal(mlab.long(), R.lowest_argmax(logits)), (what, "per-model labels are not the lowest-index argmax of the device logits")
    assert torch.equal(labels, R.smallest_mode(mlab.long(), K)), (what, "final label is not the smallest mode of the per-model labels")
    jerr = float((js.double() - R.js_formula(logits)).abs().max())
    print("pixel classifier %s: worst js error %.3e, bound %.3e (reference fp32: %.3e)" % (what, jerr, bd.js, bd.ref_js))
    assert jerr <= bd.js, (what, jerr, bd.js)
    bd.check_labels(labels, what)


@functools.lru_cache(maxsize=None)
def case_data(C_, B, H, W, M, K, f32, seed):
    """inputs, oracle and bounds of one case, computed once and shared (never modified)"""
    sds = R.gen_models(C_, M, K, seed)
    v = R.gen_features(B, C_, H, W, bool(f32), seed + 1)
    return sds, v, R.Bounds(sds, v)


# name: (C, B, H, W, M, K, fp32 map, channels-last)
CASES = {
    "C72 NCHW fp16, 63 pixels": (72, 2, 9, 7, 3, 5, 0, 0),                   # a partial pixel tile, a k tail
    "C200 channels-last fp16, large nets": (200, 2, 17, 16, 10, 34, 0, 1),   # five pixel tiles, 50 workgroups over the XCD numbering
    "C8 fp32 NCHW, one model": (8, 1, 16, 16, 1, 2, 1, 0),
    "C136 fp32 channels-last K29": (136, 2, 12, 12, 4, 29, 1, 1),            # the last small-net size
    "C136 fp32 channels-last K30": (136, 2, 12, 12, 4, 30, 1, 1),            # the first large-net size
    "C8448 fp16 NCHW": (8448, 1, 17, 16, 2, 19, 0, 0),                       # the reference's depth: 264 k-tiles
    "one row": (40, 2, 1, 37, 3, 7, 0, 0),
    "one column": (40, 2, 37, 1, 3, 7, 0, 1),
    "M16": (24, 1, 8, 9, 16, 3, 0, 0),                                       # the maximum ensemble
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_against_the_oracle(name):
    C_, B, H, W, M, K, f32, chlast = CASES[name]
    sds, v, bd = case_data(C_, B, H, W, M, K, f32, sum(map(ord, name)))
    L = _lib()
    h, _ = create(L, sds)
    try:
        d = (_cl(v) if chlast else v).cuda()
        assert d.stride() == (_cl(v) if chlast else v).stride()
        got = launch(L, h, M, K, d)
        check(got, bd, M, K, B, name)
        only = launch(L, h, M, K, d, outs=False)                             # NULL optional outputs: the logits live in the workspace
        assert torch.equal(only, got[0])
    finally:
        L.gdf_pixcls_destroy(h)


def test_the_reference_call_form_and_top_k():
    """the reference's (P, dim) matrix with strides (1, P) (task-pixel.py:100) through the Python wrapper; top_k is torch's expression on the device js"""
    from components.postproc import PixelClassifierEnsemble, predict_labels
    C_, H, W, M, K = 40, 10, 13, 3, 7
    sds, v, bd = case_data(C_, 1, H, W, M, K, 0, 707)
    d = v.cuda()
    x = d[0].view(C_, -1).permute(1, 0)
    assert x.stride() == (1, H * W)
    ens = PixelClassifierEnsemble(sds)
    labels, top_k, js, mlab, logits = ens.predict_full(x, (H, W))
    assert labels.is_cuda and js.is_cuda and top_k.is_cuda and tuple(labels.shape) == (H, W) and top_k.dim() == 0 and labels.dtype == torch.int64
    check((labels.cpu().reshape(-1), js.cpu().reshape(-1), mlab.cpu().reshape(M, -1), logits.cpu()), bd, M, K, 1, "(P, dim) matrix")
    assert torch.equal(top_k, js.reshape(-1).sort()[0][-int(H * W / 10):].mean())
    # the reference's signature: CPU labels of the given size, 0-d top_k; a list of modules is accepted and its ensemble cached
    mods = [R.Module(sd) for sd in sds]
    l2, t2 = predict_labels(mods, x, (H, W))
    assert not l2.is_cuda and l2.dtype == torch.int64 and tuple(l2.shape) == (H, W) and t2.dim() == 0
    assert torch.equal(l2, labels.cpu()) and torch.equal(t2.cpu(), top_k.cpu())
    l3, _ = predict_labels(mods, x.cpu().numpy(), (H, W))                    # numpy features, as the reference accepts
    assert torch.equal(l3, l2)
    # fewer than ten pixels: the reference's slice averages everything
    small = ens.predict_full(d[:, :, :1, :7])
    assert torch.equal(small[1][0], small[2].reshape(-1).sort()[0].mean())


def test_two_equal_classes_give_the_lower_label():
    """classes 1 and 3 are made exactly equal in every model (the same last-layer row and bias) and favoured by half a unit of bias: where they win, every model and the vote say 1"""
    C_, B, H, W, M, K = 24, 1, 8, 9, 3, 5
    sds = [dict(sd) for sd in R.gen_models(C_, M, K, 909)]
    for sd in sds:
        w, b = sd["layers.6.weight"].clone(), sd["layers.6.bias"].clone()
        b[1] += 0.5
        w[3], b[3] = w[1], b[1]
        sd["layers.6.weight"], sd["layers.6.bias"] = w, b
    v = R.gen_features(B, C_, H, W, False, 910)
    L = _lib()
    h, _ = create(L, sds)
    try:
        labels, js, mlab, logits = launch(L, h, M, K, v.cuda())
    finally:
        L.gdf_pixcls_destroy(h)
    assert torch.equal(logits[:, :, 1], logits[:, :, 3])
    assert torch.equal(mlab.long(), R.lowest_argmax(logits)) and not bool((mlab == 3).any()) and bool((mlab == 1).any())
    assert torch.equal(labels, R.smallest_mode(mlab.long(), K)) and not bool((labels == 3).any())
    # a planted tie of the vote: with M = 2 models every disagreement is a tie and the smaller label wins
    h2, _ = create(L, sds[:2])
    try:
        l2, _, m2, _ = launch(L, h2, 2, K, v.cuda())
    finally:
        L.gdf_pixcls_destroy(h2)
    assert torch.equal(l2, m2.long().min(0)[0]) and bool((m2[0] != m2[1]).any())


def test_strided_views_keep_the_nan_padding_out():
    """the map is a view into a larger NaN-filled buffer: x stride 2 inside an NCHW buffer (the any-stride path), and a channels-last buffer whose
    pixels are 8 channels longer than C (16-byte loads along C must stop at C)"""
    C_, B, H, W, M, K = 72, 2, 6, 5, 3, 5
    sds, v, bd = case_data(C_, B, H, W, M, K, 0, 1111)
    L = _lib()
    h, _ = create(L, sds)

    def nchw_view():
        buf = torch.full((B, C_ + 3, H + 2, 2 * W + 1), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, 1:C_ + 1, 1:H + 1, 1:2 * W:2]
        view.copy_(v)
        return buf, view

    def cl_view():
        buf = torch.full((B, H + 1, W + 2, C_ + 8), float("nan"), dtype=v.dtype, device="cuda")
        view = buf[:, :H, 1:W + 1, :C_].permute(0, 3, 1, 2)
        view.copy_(v)
        return buf, view

    try:
        for what, mk in (("x stride 2", nchw_view), ("padded channels-last pixels", cl_view)):
            buf, d = mk()
            assert tuple(d.shape) == (B, C_, H, W) and not d.is_contiguous() and bool(torch.isnan(buf).any())
            got = launch(L, h, M, K, d)
            assert bool(torch.isfinite(got[3]).all())
            check(got, bd, M, K, B, what)
    finally:
        L.gdf_pixcls_destroy(h)


def same_bits(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
            and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)))


def test_streams_and_determinism():
    C_, B, H, W, M, K = 200, 2, 13, 11, 4, 19
    sds, v, bd = case_data(C_, B, H, W, M, K, 0, 1212)
    L = _lib()
    h, _ = create(L, sds)
    try:
        d = v.cuda()
        first = launch(L, h, M, K, d)
        again = launch(L, h, M, K, d)
        s1 = torch.cuda.Stream()
        torch.cuda.synchronize()
        other = launch(L, h, M, K, d, st=vp(s1.cuda_stream))
        assert same_bits(again, first) and same_bits(other, first)           # the same inputs: the same bits, on any stream
        check(first, bd, M, K, B, "NCHW copy")
        check(launch(L, h, M, K, _cl(d)), bd, M, K, B, "channels-last copy")  # accepted too; equality between the two layouts is not required
    finally:
        L.gdf_pixcls_destroy(h)


def test_beside_a_gemm_on_a_second_stream_keeps_its_bits():
    """one call while a GEMM runs on a second stream: the bits equal the solo run.  Once, no loop."""
    C_, B, H, W, M, K = 320, 2, 32, 32, 10, 19
    sds = R.gen_models(C_, M, K, 1313)
    L = _lib()
    h, _ = create(L, sds)
    try:
        d = R.gen_features(B, C_, H, W, False, 1314).cuda()
        dcl = _cl(d)
        solo, solo_cl = launch(L, h, M, K, d), launch(L, h, M, K, dcl)
        n = 4096
        g = torch.Generator().manual_seed(0)
        A = (torch.randn(n, n, generator=g) * 0.1).half().cuda()
        Wt = (torch.randn(n, n, generator=g) * 0.1).half().cuda()
        o16 = torch.zeros(n, n, dtype=torch.half, device="cuda")
        s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(6):                                                   # a few milliseconds of GEMM queued on s1, then the two calls on s0
            ok(L.gdf_op_gemm(P(A), n, P(Wt), None, None, None, 0, P(o16), n, None, 0, n, n, n, 0, vp(s1.cuda_stream)), L)
        beside = launch(L, h, M, K, d, st=vp(s0.cuda_stream))
        beside_cl = launch(L, h, M, K, dcl, st=vp(s0.cuda_stream))
        assert same_bits(beside, solo) and same_bits(beside_cl, solo_cl)
        assert bool(torch.isfinite(o16.float()).all())
    finally:
        L.gdf_pixcls_destroy(h)


def test_refusals_and_the_empty_batch_launch_nothing():
    L = _lib()
    sds = R.gen_models(8, 2, 3, 1414)
    h, ens = create(L, sds)
    d = R.gen_features(2, 8, 4, 4, False, 1415).cuda()
    labels = torch.full((32,), PAT64, dtype=torch.int64, device="cuda")
    js = guard((32,), torch.float32)
    nbytes = L.gdf_pixcls_workspace(h, 2, 4, 4)
    ws = torch.full((nbytes + 16,), PAT8, dtype=torch.uint8, device="cuda")
    src = R.agg_src(d.data_ptr(), 0, d.stride(), d.shape)

    def call(handle=h, B=2, nb=nbytes, lab=labels, wsp=None):
        return L.gdf_pixcls_predict(handle, ctypes.addressof(src), B, P(lab) if lab is not None else None, P(js), None, None,
                                    wsp if wsp is not None else P(ws), nb, stream())
    try:
        assert call(handle=None) == R.GDF_ERR_ARG and call(lab=None) == R.GDF_ERR_ARG and call(nb=nbytes - 1) == R.GDF_ERR_ARG
        assert call(B=-1) == R.GDF_ERR_ARG and call(wsp=vp(ws.data_ptr() + 8)) == R.GDF_ERR_ARG
        assert b"gdf_pixcls_predict" in L.gdf_last_error()
        src.C = 9
        assert call() == R.GDF_ERR_ARG
        src.C = 8
        src.H = 0
        assert call() == R.GDF_ERR_ARG
        src.H = 4
        assert call(B=0) == 0
        torch.cuda.synchronize()
        assert bool((labels.cpu() == PAT64).all()) and bool(is_guard(js.cpu()).all()) and bool((ws.cpu() == PAT8).all())
        # creation: outside the limits is unsupported, nonsense is an argument error; no handle comes back
        f = [vp(t.data_ptr()) for t in ens.folded]
        out = vp()
        assert L.gdf_pixcls_create(8, 17, 128, 32, 3, *f, ctypes.byref(out)) == R.GDF_ERR_UNSUPPORTED and not out.value
        assert L.gdf_pixcls_create(8, 2, 128, 32, 65, *f, ctypes.byref(out)) == R.GDF_ERR_UNSUPPORTED
        assert L.gdf_pixcls_create(8, 2, 288, 32, 3, *f, ctypes.byref(out)) == R.GDF_ERR_UNSUPPORTED
        assert L.gdf_pixcls_create(8, 2, 100, 32, 3, *f, ctypes.byref(out)) == R.GDF_ERR_UNSUPPORTED
        assert L.gdf_pixcls_create(0, 2, 128, 32, 3, *f, ctypes.byref(out)) == R.GDF_ERR_ARG
        assert L.gdf_pixcls_create(8, 2, 128, 32, 3, None, *f[1:], ctypes.byref(out)) == R.GDF_ERR_ARG and not out.value
        assert L.gdf_pixcls_workspace(None, 2, 4, 4) == 0
    finally:
        L.gdf_pixcls_destroy(h)


def test_widths_between_the_two_architectures_are_padded():
    """h1 = 64, h2 = 64: inside the limits, served by the (256, 128) instantiation with zero padding"""
    C_, M, K, H, W = 40, 2, 6, 8, 9
    g = torch.Generator().manual_seed(1515)
    W1, b1 = 1.5 * torch.randn(M, 64, C_, generator=g) / C_ ** 0.5, 0.3 * torch.randn(M, 64, generator=g)
    W2, b2 = 1.5 * torch.randn(M, 64, 64, generator=g) / 8, 0.3 * torch.randn(M, 64, generator=g)
    W3, b3 = 1.5 * torch.randn(M, K, 64, generator=g) / 8, 0.3 * torch.randn(M, K, generator=g)
    v = R.gen_features(1, C_, H, W, False, 1516)
    x = R.rows(v).double()
    want = torch.stack([torch.relu(torch.relu(x @ W1[m].double().T + b1[m].double()) @ W2[m].double().T + b2[m].double()) @ W3[m].double().T
                        + b3[m].double() for m in range(M)])
    L = _lib()
    h = vp()
    ok(L.gdf_pixcls_create(C_, M, 64, 64, K, *[vp(t.contiguous().data_ptr()) for t in (W1, b1, W2, b2, W3, b3)], ctypes.byref(h)), L)
    try:
        _, _, _, logits = launch(L, h, M, K, v.cuda())
    finally:
        L.gdf_pixcls_destroy(h)
    x32 = R.rows(v).float()
    ref = torch.stack([torch.relu(torch.relu(x32 @ W1[m].T + b1[m]) @ W2[m].T + b2[m]) @ W3[m].T + b3[m] for m in range(M)])
    bound = R.MARGIN * float(R.block_rel(ref, want).max())                   # the same rule: 8 x torch's fp32 error on this network
    assert float(R.block_rel(logits, want).max()) <= bound


def test_python_wrappers_agree_with_the_c_call():
    import diffusion_feature
    from components.postproc import PixelClassifierEnsemble, aggregate
    C_, B, H, W, M, K = 72, 2, 9, 7, 3, 5
    sds, v, bd = case_data(C_, B, H, W, M, K, 0, sum(map(ord, "C72 NCHW fp16, 63 pixels")))
    L = _lib()
    h, _ = create(L, sds)
    try:
        d = _cl(v).cuda()
        want = launch(L, h, M, K, d)
    finally:
        L.gdf_pixcls_destroy(h)
    ens = PixelClassifierEnsemble(sds)
    labels, top_k, js, mlab, logits = ens.predict_full(d)
    assert labels.is_cuda and tuple(labels.shape) == (B, H, W) and tuple(top_k.shape) == (B,) and tuple(mlab.shape) == (M, B, H, W)
    assert same_bits((labels.cpu().reshape(-1), js.cpu().reshape(-1), mlab.cpu().reshape(M, -1), logits.cpu()), want)
    for b in range(B):
        assert torch.equal(top_k[b], js[b].reshape(-1).sort()[0][-int(H * W / 10):].mean())
    l2, t2 = ens.predict(d)
    assert torch.equal(l2, labels) and torch.equal(t2, top_k)
    # FeatureExtractor.segment = aggregate, then predict
    fe = diffusion_feature.FeatureExtractor.__new__(diffusion_feature.FeatureExtractor)
    feats = {"a": d[:, :40], "b": torch.nn.functional.avg_pool2d(d[:, 40:].float(), 2, ceil_mode=True).half()}
    agg = aggregate(list(feats.values()), (12, 10))
    la, ta = ens.predict(agg)
    ls, ts = fe.segment(ens, feats, (12, 10))
    assert tuple(ls.shape) == (B, 12, 10) and torch.equal(ls, la) and torch.equal(ts, ta)
    ll, tl = fe.segment([R.Module(sd) for sd in sds], feats, (12, 10))       # the reference's list of modules
    assert torch.equal(ll, la) and torch.equal(tl, ta)


@pytest.mark.parametrize("name", ["small", "large"])
def test_reference_results_on_the_device(name):
    from components.postproc import predict_labels, PixelClassifierEnsemble
    from test_pixel_classifier_cpu import as_map, golden
    sds, x, size, want_labels, want_top_k = golden(name)
    bd = R.Bounds(sds, as_map(x, size))
    labels, top_k = predict_labels(PixelClassifierEnsemble(sds), x, size)    # host features are moved to the device, as the reference moves them
    assert not labels.is_cuda and tuple(labels.shape) == size
    bd.check_labels(labels, "golden on the device, " + name)
    clear = ~bd.ambiguous.reshape(size)
    assert torch.equal(labels[clear], want_labels[clear]) and top_k.dim() == 0
