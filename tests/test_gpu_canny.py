"""Kernel-level tests of the device Canny (-m gpu): gdf_op_canny_classify, gdf_op_canny_link and the fused gdf_op_canny (csrc/canny.hip,
include/gdf_ops.h) against the NumPy restatement of cv::Canny in tests/canny_oracle.py.  Everything is compared for EQUALITY.  Guard sentinels
around every buffer, inputs unchanged after the call, and a second launch gives the same bits.

Shapes: the classify tile is 16 rows x 64 columns, the linking tile 32 x 32.  (1, 1, 1), (1, 2, 7), (1, 8, 8): images smaller than any halo;
(2, 37, 53): two images, more than one tile of either kind in y, odd everything, H W % 4 != 0 (the scalar store paths); (1, 96, 160): the size the
statistics below are asserted at (it divides the linking tile: seams everywhere, no partial tile); (1, 130, 257): more than one tile in both
directions of both kinds, dividing neither."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import canny_oracle as O

pytestmark = pytest.mark.gpu
vp = C.c_void_p
GUARD = 64                        # sentinel elements in front of and behind every buffer (keeps the payload 16-byte aligned)
SHAPES = [(1, 1, 1), (1, 2, 7), (1, 8, 8), (2, 37, 53), (1, 96, 160), (1, 130, 257)]
KINDS = {"u8_hwc3": 0, "u8_hw": 1, "f32_nchw": 2, "f16_nchw": 3}


def _lib():
    from components import native
    return native.load_library()


def _guarded(vals, sentinel):
    """(whole buffer, payload view) of a flat device copy of `vals` (a torch tensor) with GUARD sentinel elements on both sides"""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=vals.dtype, device="cuda")
    buf[GUARD:GUARD + n] = vals.reshape(-1).cuda()
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, sentinel):
    return bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == sentinel).all())


def _workspace(L, B, H, W):
    n = L.gdf_op_canny_workspace_bytes(B, H, W)
    assert n > 0
    return _guarded(torch.full((n,), 0xA5, dtype=torch.uint8), 0x5A)       # stale garbage inside: nothing may be assumed of it


@functools.lru_cache(maxsize=None)
def _images(shape):
    B, H, W = shape
    return O.smooth_noise(B, H, W, seed=100 * H + W)                        # (B, H, W, 3) uint8


def _exact_ties():
    """fp32 values x for which (x / 2 + 0.5) * 255, every step rounded to fp32, is exactly k + 0.5: half-to-even decides their byte"""
    out = []
    for k in range(0, 255, 7):
        x0 = np.float32(2.0 * (k + 0.5) / 255.0 - 1.0)
        for step in range(-3, 4):
            x = x0
            for _ in range(abs(step)):
                x = np.nextafter(x, np.float32(2.0 if step > 0 else -2.0), dtype=np.float32)
            v = (np.float32(x) / np.float32(2) + np.float32(0.5)) * np.float32(255)
            if float(v) == k + 0.5:
                out.append(float(x))
                break
    return out


@functools.lru_cache(maxsize=None)
def _source(shape, kind):
    """(source tensor as the entry takes it, the uint8 images (B, H, W[, 3]) the oracle sees)"""
    img = torch.from_numpy(_images(shape))
    if kind == "u8_hwc3":
        return img, img.numpy()
    if kind == "u8_hw":
        return img[..., 1].contiguous(), img[..., 1].contiguous().numpy()
    # tensors in [-1.1, 1.1] (both clamps act) off the byte lattice, with exact rounding ties planted where there is room
    g = torch.Generator().manual_seed(7)
    t = ((img.float() / 255 * 2 - 1) * 1.1 + 0.003 * torch.randn(img.shape, generator=g)).permute(0, 3, 1, 2).contiguous()
    ties = torch.tensor(_exact_ties(), dtype=torch.float32)
    if kind == "f32_nchw" and t[0, 0].numel() >= ties.numel():
        assert ties.numel() >= 8
        t[0, 0].view(-1)[:ties.numel()] = ties
    if kind == "f16_nchw":
        t = t.half()
    return t, O.quantise(t).permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def _oracle_cls(shape, kind, low, high):
    return np.stack([O.classify(im, low, high) for im in _source(shape, kind)[1]])


@functools.lru_cache(maxsize=None)
def _oracle_edges(shape, kind):
    return np.stack([O.link(c) for c in _oracle_cls(shape, kind, 100, 200)])


def _classify(L, src, kind, shape, low, high):
    B, H, W = shape
    sb, sv = _guarded(src, 3)
    outs = []
    for _ in range(2):
        cb, cv = _guarded(torch.full((B * H * W,), 7, dtype=torch.uint8), 9)
        assert L.gdf_op_canny_classify(vp(sv.data_ptr()), KINDS[kind], B, H, W, low, high, vp(cv.data_ptr()), None) == 0, L.gdf_last_error()
        torch.cuda.synchronize()
        assert _intact(cb, 9)
        outs.append(cv.cpu().numpy().reshape(B, H, W))
    assert _intact(sb, 3) and torch.equal(sv.cpu(), src.reshape(-1))         # the source is read only
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_classify_equals_the_oracle(shape, kind):
    L = _lib()
    src, _ = _source(shape, kind)
    for low, high in ((100, 200), (200, 100)):                               # the second pair: swapped by the entry
        want = _oracle_cls(shape, kind, low, high)
        got = _classify(L, src, kind, shape, low, high)
        assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    if shape[1] >= 96:                                                       # the images are not trivial: asserted on the ORACLE's output
        cls, e = _oracle_cls(shape, kind, 100, 200), _oracle_edges(shape, kind)
        for c, ee in zip(cls, e):
            st = O.link_stats(c, ee)
            assert st["strong"] >= 0.01 * c.size and st["kept"] >= 50 and st["dropped"] >= 50, st


def test_classify_low_contrast_steps_and_channel_ties():
    L = _lib()
    # lower contrast: candidates but no strong pixel at all -> everything is dropped
    low = O.smooth_noise(1, 96, 160, sigma=3.0, contrast=0.35, seed=11)
    cls = O.classify(low[0])
    assert int((cls == O.STRONG).sum()) == 0 and int((cls == O.CANDIDATE).sum()) >= 50
    assert np.array_equal(_classify(L, torch.from_numpy(low), "u8_hwc3", (1, 96, 160), 100, 200)[0], cls)
    assert not _fused(L, torch.from_numpy(low), "u8_hwc3", (1, 96, 160), 0).any()
    # the hand-checkable step images
    for name, (img, want) in O.steps().items():
        H, W = img.shape[:2]
        src = torch.from_numpy(img)[None].contiguous()
        assert np.array_equal(_classify(L, src, "u8_hwc3", (1, H, W), 100, 200)[0], O.classify(img)), name
        assert np.array_equal(_fused(L, src, "u8_hwc3", (1, H, W), 0)[0] > 0, want), name
    # channel ties: channels 0 and 1 have equal magnitudes everywhere and dy of opposite sign; the first channel must win.  Swapping the two
    # channels changes the oracle's map at hundreds of pixels: the rule shows.
    img = O.ties_image()
    H, W = img.shape[:2]
    m0, m1 = O.sobel(img[..., 0])[0], O.sobel(img[..., 1])[0]
    assert int(((m0 == m1) & (m0 > 100)).sum()) >= 1000
    want = O.classify(img)
    assert int((want != O.classify(img[..., [1, 0, 2]])).sum()) >= 100
    assert np.array_equal(_classify(L, torch.from_numpy(img)[None].contiguous(), "u8_hwc3", (1, H, W), 100, 200)[0], want)


def _link(L, cls, dst_kind=0):
    """cls uint8 (B, H, W) numpy -> the entry's output (numpy): uint8 (B, H, W) or fp16 (B, 3, H, W)"""
    B, H, W = cls.shape
    src = torch.from_numpy(np.ascontiguousarray(cls))
    cb, cv = _guarded(src, 3)
    outs = []
    for _ in range(2):
        wb, wv = _workspace(L, B, H, W)
        if dst_kind == 0:
            ob, ov = _guarded(torch.full((B * H * W,), 77, dtype=torch.uint8), 99)
        else:
            ob, ov = _guarded(torch.full((B * 3 * H * W,), 5.0, dtype=torch.float16), -3.0)
        assert L.gdf_op_canny_link(vp(cv.data_ptr()), B, H, W, vp(ov.data_ptr()), dst_kind, vp(wv.data_ptr()), None) == 0, L.gdf_last_error()
        torch.cuda.synchronize()
        assert _intact(ob, 99 if dst_kind == 0 else -3.0) and _intact(wb, 0x5A)
        outs.append(ov.cpu().numpy().reshape((B, H, W) if dst_kind == 0 else (B, 3, H, W)))
    assert _intact(cb, 3) and torch.equal(cv.cpu(), src.reshape(-1))
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def _two_images():
    """image 0: a strong component that touches its last row; image 1: candidates on its first row, and nothing strong -> they stay unlinked.
    Also in image 0: a strong pixel at the end of a row and a candidate at the start of the next (adjacent indices, not neighbours)."""
    H, W = 96, 160
    a = np.full((2, H, W), O.NONE, np.uint8)
    a[0, H - 1, :] = O.CANDIDATE
    a[0, H - 1, 5] = O.STRONG
    a[1, 0, :] = O.CANDIDATE
    a[1, 1, W - 1] = O.CANDIDATE
    a[0, 10, W - 1] = O.STRONG
    a[0, 11, 0] = O.CANDIDATE
    return a


def _two_components():
    """two components one class-1 pixel apart (a column of NONE between two candidate bands, across a tile seam), one of them with a strong pixel"""
    a = np.full((1, 96, 160), O.NONE, np.uint8)
    a[0, 8:80, 30] = O.CANDIDATE
    a[0, 8:80, 32] = O.CANDIDATE
    a[0, 40, 32] = O.STRONG
    a[0, 31, 60:100] = O.CANDIDATE           # and the same across a horizontal seam: row 32 empty, row 33 with the strong pixel
    a[0, 33, 60:100] = O.CANDIDATE
    a[0, 33, 99] = O.STRONG
    return a


LINK_MAPS = {
    "serpentine": lambda: O.serpentine()[None],
    "serpentine-without-strong": lambda: O.serpentine(strong=False)[None],
    "diagonals-across-tile-corners": lambda: O.diagonal()[None],
    "two-components-one-pixel-apart": _two_components,
    "two-images-stay-unlinked": _two_images,
    "random-0.30": lambda: O.random_map(96, 160, 0.30, 0.002, 1)[None],
    "random-0.42": lambda: O.random_map(96, 160, 0.42, 0.002, 2)[None],
    "random-0.55": lambda: O.random_map(96, 160, 0.55, 0.002, 3)[None],
    "random-0.42-2x37x53": lambda: np.stack([O.random_map(37, 53, 0.42, 0.01, 4), O.random_map(37, 53, 0.42, 0.01, 5)]),
    "random-0.42-130x257": lambda: O.random_map(130, 257, 0.42, 0.002, 6)[None],
    "1x1-strong": lambda: np.full((1, 1, 1), O.STRONG, np.uint8),
    "2x7": lambda: np.array([[[0, 0, 1, 0, 2, 1, 0], [1, 1, 1, 1, 1, 1, 1]]], np.uint8),
}


@pytest.mark.parametrize("name", list(LINK_MAPS))
def test_link_equals_the_oracle(name):
    L = _lib()
    cls = LINK_MAPS[name]()
    want = np.stack([O.link(c) for c in cls])
    if name == "serpentine":
        assert int((want > 0).sum()) == int((cls != O.NONE).sum()) == 7727                          # every pixel of the path is output
    if name == "serpentine-without-strong":
        assert not want.any()
    if name == "two-images-stay-unlinked":
        assert (want[0, 95] == 255).all() and not want[1].any() and want[0, 10, 159] == 255 and want[0, 11, 0] == 0
    if name == "two-components-one-pixel-apart":
        assert not want[0, :, 30].any() and (want[0, 8:80, 32] == 255).all() and not want[0, 31, 60:100].any() and (want[0, 33, 60:100] == 255).all()
    if name.startswith("random-0.") and cls.shape[1:] == (96, 160):
        st = O.link_stats(cls[0], want[0])
        assert st["kept"] >= 50 and st["dropped"] >= 50, st
    got = _link(L, cls)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    if name in ("random-0.42", "random-0.42-2x37x53"):                          # the control form: H W % 4 == 0 and != 0
        got16 = _link(L, cls, dst_kind=1)
        assert got16.dtype == np.float16 and np.array_equal(got16, np.repeat((want[:, None] > 0).astype(np.float16), 3, axis=1))


def _fused(L, src, kind, shape, dst_kind, stream=None):
    B, H, W = shape
    sb, sv = _guarded(src, 3)
    wb, wv = _workspace(L, B, H, W)
    if dst_kind == 0:
        ob, ov = _guarded(torch.full((B * H * W,), 77, dtype=torch.uint8), 99)
    else:
        ob, ov = _guarded(torch.full((B * 3 * H * W,), 5.0, dtype=torch.float16), -3.0)
    rc = L.gdf_op_canny(vp(sv.data_ptr()), KINDS[kind], B, H, W, 100, 200, vp(ov.data_ptr()), dst_kind, vp(wv.data_ptr()),
                        vp(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, L.gdf_last_error()
    torch.cuda.synchronize()
    assert _intact(ob, 99 if dst_kind == 0 else -3.0) and _intact(wb, 0x5A) and _intact(sb, 3) and torch.equal(sv.cpu(), src.reshape(-1))
    return ov.cpu().numpy().reshape((B, H, W) if dst_kind == 0 else (B, 3, H, W))


@pytest.mark.parametrize("kind", ["u8_hwc3", "f32_nchw"])
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 96, 160)], ids=lambda s: "%dx%dx%d" % s)
def test_fused_equals_link_of_classify(shape, kind):
    from PIL import Image
    from components.control import control_tensor
    L = _lib()
    src, u8 = _source(shape, kind)
    want = _oracle_edges(shape, kind)
    got = _fused(L, src, kind, shape, 0)
    assert np.array_equal(got, want)
    assert np.array_equal(got, _link(L, _classify(L, src, kind, shape, 100, 200)))
    assert np.array_equal(_fused(L, src, kind, shape, 0), got)                  # a second call, a fresh workspace full of garbage: same bits
    # the control form == control_tensor of the reference's three-channel edge image (controlnet.py:30-36)
    pil = [Image.fromarray(np.concatenate([e[:, :, None]] * 3, axis=2)) for e in want]
    ctl = control_tensor(pil, shape[1], shape[2])
    got16 = torch.from_numpy(_fused(L, src, kind, shape, 1))
    assert ctl.dtype == got16.dtype == torch.float16 and torch.equal(got16, ctl)
    # and through components/native.py canny on the current stream
    from components import native
    assert torch.equal(native.canny(src.cuda(), 100, 200, out="control").cpu(), ctl)
    assert np.array_equal(native.canny(src.cuda(), 200, 100.5, out="u8").cpu().numpy(), want)


def test_batch_position_does_not_matter():
    """the same image at batch positions 0 and 2 gives the same bits (labels are global over the batch; results are not)"""
    L = _lib()
    a, b = _images((1, 96, 160))[0], _images((1, 130, 257))[0][:96, :160]
    src = torch.from_numpy(np.stack([a, b, a]))
    got = _fused(L, src, "u8_hwc3", (3, 96, 160), 0)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], _oracle_edges((1, 96, 160), "u8_hwc3")[0]) and np.array_equal(got[1], O.canny(b))


def test_beside_another_stream():
    """one fused call while a GEMM runs on a second stream: the bits equal the solo run.  Once, no loop."""
    from ops_binding import P, lib, ok
    Lg = lib()
    L = _lib()
    shape, kind = (1, 130, 257), "u8_hwc3"
    src, _ = _source(shape, kind)
    solo = _fused(L, src, kind, shape, 0)
    M, N, K = 4096, 4096, 4096
    g = torch.Generator().manual_seed(0)
    A = (torch.randn(M, K, generator=g) * 0.1).half().cuda()
    Wt = (torch.randn(N, K, generator=g) * 0.1).half().cuda()
    o16 = torch.zeros(M, N, dtype=torch.half, device="cuda")
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(4):                                                          # a few milliseconds of GEMM queued on s1, then the Canny on s0
        ok(Lg.gdf_op_gemm(P(A), K, P(Wt), None, None, None, 0, P(o16), N, None, 0, M, N, K, 0, vp(s1.cuda_stream)), Lg)
    with torch.cuda.stream(s0):
        beside = _fused(L, src, kind, shape, 0, stream=s0)
    torch.cuda.synchronize()
    assert np.array_equal(beside, solo) and np.array_equal(solo, _oracle_edges(shape, kind))
    assert bool(torch.isfinite(o16.float()).all())
