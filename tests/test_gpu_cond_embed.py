"""Kernel-level parity of the ControlNet conditioning-embedding conv (-m gpu): cond_conv3x3_kernel (csrc/cond_embed.hip) through
gdf_op_cond_conv3x3 (include/gdf_ops.h), every (Cin, Cout, stride, SiLU) form a ControlNet plan launches — the seven layers of the chain and
the 256 -> block_out_channels[0] conv_out — plus conv_out's add-into-destination form, against float64 F.conv2d on the same fp16 inputs."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
vp, ci = C.c_void_p, C.c_int
GUARD = 64                       # sentinel elements in front of and behind every buffer (keeps the payload 16-byte aligned)
TOL16 = 1e-3                     # tests/test_gpu_gemm.py: relative L2 per 16 x 16 block of an fp16 output
PADC = 8                         # sentinel columns behind the channels of every pixel: ldx = Cin + 8, ldo = Cout + 8
X_SENT, O_SENT = 333.0, -7.0

# (Cin, Cin of the checkpoint, Cout, stride, silu, add_into): the table of the embedding, conv_out at two widths, and its add-into form
FORMS = [(8, 3, 16, 1, 1, 0), (16, 16, 16, 1, 1, 0), (16, 16, 32, 2, 1, 0), (32, 32, 32, 1, 1, 0), (32, 32, 96, 2, 1, 0), (96, 96, 96, 1, 1, 0),
         (96, 96, 256, 2, 1, 0), (256, 256, 64, 1, 0, 0), (256, 256, 320, 1, 0, 0), (256, 256, 320, 1, 0, 1)]
# borders everywhere (8 x 8), tiles that do not divide (1920 = 7.5 x 256 pixels), non-square, more than one workgroup
IMAGES = [(1, 8, 8), (2, 24, 40), (1, 16, 72)]


def _lib():
    from components import native
    L = native.load_library()
    L.gdf_op_cond_conv3x3.restype, L.gdf_op_cond_conv3x3.argtypes = ci, [vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp, ci, ci, vp]
    L.gdf_op_cond_weight_bytes.restype, L.gdf_op_cond_weight_bytes.argtypes = C.c_size_t, [ci, ci]
    L.gdf_op_cond_pack_weights.restype, L.gdf_op_cond_pack_weights.argtypes = ci, [vp, ci, vp, ci, ci, ci, vp]
    L.gdf_op_cond_pack_image.restype, L.gdf_op_cond_pack_image.argtypes = ci, [vp, ci, ci, ci, ci, ci, vp, vp]
    return L


def _guarded(vals, sentinel, dtype=torch.float16):
    """(whole buffer, payload view) of a flat device copy of `vals` with GUARD sentinel elements on both sides"""
    n = vals.numel()
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = vals.reshape(-1).to("cuda", dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, sentinel):
    return bool((torch.cat([buf[:GUARD], buf[-GUARD:]]) == sentinel).all())


def _pack(L, w_oihw, cin):
    co, ci_src = w_oihw.shape[:2]
    nb = L.gdf_op_cond_weight_bytes(cin, co)
    assert nb == (9 * cin + 31) // 32 * 32 * co * 2
    wb, w = _guarded(w_oihw, 5.0)
    pb, pk = _guarded(torch.zeros(nb // 2), -9.0)
    assert L.gdf_op_cond_pack_weights(vp(w.data_ptr()), 0, vp(pk.data_ptr()), co, ci_src, cin, None) == 0, L.gdf_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(pb, -9.0) and _guards_intact(wb, 5.0)
    return pb, pk


def _blocks(t):
    """(rows, cols) float64 -> per 16 x 16 block sums of squares"""
    pr, pc = -t.shape[0] % 16, -t.shape[1] % 16
    t = F.pad(t, (0, pc, 0, pr))
    return t.reshape(t.shape[0] // 16, 16, t.shape[1] // 16, 16).pow(2).sum((1, 3))


@pytest.mark.parametrize("img", IMAGES, ids=lambda i: "%dx%dx%d" % i)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%d-%d-s%d%s%s" % (f[0], f[2], f[3], "-silu" if f[4] else "", "-add" if f[5] else ""))
def test_cond_conv3x3(form, img):
    """Per 16 x 16 block of the [pixels][Cout] result: relative L2 <= 1e-3.  Per element:
        |got - ref| <= 2^-11 |ref| + 2^-11 * sum|x||w| * 2^-12 + 2^-24
    one fp16 rounding of the output (half an ulp is at most 2^-11 |ref|), the fp32 accumulation of the dot product (a multiple of 2^-24 of
    sum|x||w|, here 2: generous by a constant for the MFMA's pairwise sums over K = 9 Cin <= 2304 terms of random signs), and the subnormal
    spacing.  Sentinel columns behind the channels of every input and output pixel, guards around every buffer, inputs unchanged, and a second
    launch gives the same bits."""
    cin, cin_src, cout, stride, silu, add = form
    B, H, W = img
    L = _lib()
    g = torch.Generator().manual_seed(1000 * cin + cout + 7 * H + stride + add)
    x = torch.randn(B, H, W, cin, generator=g).half()                    # (the first layer: channels 3..7 are garbage the zero weights must ignore)
    w = (torch.randn(cout, cin_src, 3, 3, generator=g) / (9 * cin_src) ** 0.5).half()
    bias = 0.5 * torch.randn(cout, generator=g)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    old = torch.randn(B, OH, OW, cout, generator=g).half() if add else None
    xd = x.double()[..., :cin_src].permute(0, 3, 1, 2)
    ref = F.conv2d(xd, w.double(), bias.double(), stride=stride, padding=1)
    mag = F.conv2d(xd.abs(), w.double().abs(), None, stride=stride, padding=1)
    if silu:
        ref = ref * torch.sigmoid(ref)
    if add:
        ref = ref + old.double().permute(0, 3, 1, 2)
    ref, mag = (t.permute(0, 2, 3, 1).reshape(-1, cout) for t in (ref, mag))
    assert ref.shape[0] == B * OH * OW

    ldx, ldo = cin + PADC, cout + PADC
    xrow = torch.full((B, H, W, ldx), X_SENT, dtype=torch.float16)
    xrow[..., :cin] = x
    orow = torch.full((B, OH, OW, ldo), O_SENT, dtype=torch.float16)
    if add:
        orow[..., :cout] = old
    xb, xv = _guarded(xrow, 11.0)
    bb, bv = _guarded(bias, 13.0, torch.float32)
    pb, pk = _pack(L, w, cin)
    pk0 = pk.clone()
    outs = []
    for _ in range(2):
        ob, ov = _guarded(orow, 17.0)
        rc = L.gdf_op_cond_conv3x3(vp(xv.data_ptr()), B, H, W, cin, ldx, vp(pk.data_ptr()), vp(bv.data_ptr()), cout, stride, silu, vp(ov.data_ptr()),
                                   ldo, add, None)
        assert rc == 0, L.gdf_last_error()
        torch.cuda.synchronize()
        assert _guards_intact(ob, 17.0)
        outs.append(ov.view(-1, ldo).cpu())
    assert _guards_intact(xb, 11.0) and _guards_intact(bb, 13.0) and _guards_intact(pb, -9.0)
    assert torch.equal(xv.cpu(), xrow.reshape(-1)) and torch.equal(bv.cpu(), bias) and torch.equal(pk, pk0)      # inputs are read only
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:, cout:] == O_SENT).all())                                                              # sentinel columns survive
    got = outs[0][:, :cout].double()
    assert bool(torch.isfinite(got).all())
    rel = (_blocks(got - ref) / _blocks(ref)).sqrt()
    err = (got - ref).abs()
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -11 * mag * 2.0 ** -12 + 2.0 ** -24
    print(f"cond_conv {form} {img}: worst 16x16 block {float(rel.max()):.2e}, worst element error / bound {float((err / bound).max()):.3f}")
    assert float(rel.max()) <= TOL16, float(rel.max())
    assert bool((err <= bound).all()), float((err - bound).max())


def test_cond_conv3x3_rejects_bad_arguments():
    """channel counts outside the list, odd H or W at stride 2, misaligned pointers, ld < C or no multiple of 8, a stride that is neither 1 nor
    2: an error with a message, and nothing is launched (the output keeps its sentinel)"""
    L = _lib()
    xb, x = _guarded(torch.zeros(1, 10, 10, 96), 11.0)
    ob, o = _guarded(torch.full((1, 10, 10, 256), O_SENT), 17.0)
    pb, pk = _guarded(torch.ones(9 * 96 * 256), -9.0)
    bb, bias = _guarded(torch.zeros(256), 13.0, torch.float32)
    ok = dict(x=x.data_ptr(), B=1, H=10, W=10, Cin=32, ldx=32, w=pk.data_ptr(), bias=bias.data_ptr(), Cout=32, stride=1, silu=1, out=o.data_ptr(), ldo=32,
              add=0)

    def run(**kw):
        a = dict(ok, **kw)
        return L.gdf_op_cond_conv3x3(vp(a["x"]), a["B"], a["H"], a["W"], a["Cin"], a["ldx"], vp(a["w"]), vp(a["bias"]), a["Cout"], a["stride"], a["silu"],
                                     vp(a["out"]), a["ldo"], a["add"], None)
    for bad in (dict(Cin=24, ldx=24), dict(Cout=48, ldo=48), dict(Cin=8, ldx=8, Cout=32), dict(Cin=96, ldx=96, Cout=32), dict(Cin=64, ldx=64, Cout=64, ldo=64),
                dict(Cin=256, ldx=256, Cout=96, ldo=96), dict(stride=2, H=9), dict(stride=2, W=7), dict(stride=3), dict(stride=0),
                dict(x=x.data_ptr() + 2), dict(out=o.data_ptr() + 8), dict(w=pk.data_ptr() + 4), dict(bias=bias.data_ptr() + 4),
                dict(ldx=24), dict(ldo=24), dict(ldx=36), dict(ldo=36), dict(x=0), dict(out=0), dict(w=0), dict(B=0), dict(H=0)):
        assert run(**bad) != 0, bad
        assert b"gdf_op_cond_conv3x3" in L.gdf_last_error(), bad
    torch.cuda.synchronize()
    assert bool((o == O_SENT).all()) and _guards_intact(ob, 17.0) and _guards_intact(xb, 11.0)
    assert L.gdf_op_cond_weight_bytes(24, 32) == 0
    assert L.gdf_op_cond_pack_weights(vp(pk.data_ptr()), 0, vp(pk.data_ptr()), 32, 40, 32, None) != 0
    assert run() == 0                                                       # the accepted form of the same buffers launches
    torch.cuda.synchronize()
    assert not bool((o.view(-1)[:3200] == O_SENT).any()) and bool((o.view(-1)[3200:] == O_SENT).all()) and _guards_intact(ob, 17.0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_cond_pack_image(dtype):
    """the control image NCHW in [0, 1], fp16 or fp32 -> NHWC pixels of 8 fp16 channels, channels 3..7 zero; guards intact"""
    L = _lib()
    g = torch.Generator().manual_seed(5)
    img = (torch.randint(0, 256, (2, 3, 24, 40), generator=g).float() / 255).to(dtype)
    ib, iv = _guarded(img, 3.0, dtype)
    ob, ov = _guarded(torch.full((2, 24, 40, 8), 9.0), 17.0)
    assert L.gdf_op_cond_pack_image(vp(iv.data_ptr()), 0 if dtype == torch.float16 else 1, 2, 3, 24, 40, vp(ov.data_ptr()), None) == 0, L.gdf_last_error()
    torch.cuda.synchronize()
    got = ov.view(2, 24, 40, 8).cpu()
    assert _guards_intact(ob, 17.0) and _guards_intact(ib, 3.0)
    assert torch.equal(got[..., :3], img.half().permute(0, 2, 3, 1)) and bool((got[..., 3:] == 0).all())
    assert L.gdf_op_cond_pack_image(vp(iv.data_ptr()), 2, 2, 3, 24, 40, vp(ov.data_ptr()), None) != 0          # bf16 images are not taken
    assert L.gdf_op_cond_pack_image(vp(iv.data_ptr()), 0, 2, 9, 24, 40, vp(ov.data_ptr()), None) != 0
