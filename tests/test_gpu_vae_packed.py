"""The Flux latent-preparation tail (-m gpu): gdf_op_vae_finish_packed (csrc/dit.hip vae_finish_packed_kernel) — posterior sample, shift and
scale, flow-matching noise and 2x2 packing in one pass over the fp32 moments, for up to 16 latent channels, in fp16 or bf16.

 * against float64 with the packing written as an index expression, in the manner of test_gpu_glue.py::test_vae_finish: the same input recipe
   (logvar crossing both clamp limits, no cancelling sums — asserted on the inputs, |shift| counted among the magnitudes) and the same bound,
   at most 1 ulp of the output type.  That test derives the bound for dot products of <= 16 terms; with L = 16 and quant_conv they have 32:
   the fp32 value is within 8 * (32 + 8) * 2^-24 + (exp: 0.5 * 2^-13.5 from its argument, a 32-term sum of magnitude <= 45, + 2 ulp)
   = 1.9e-5 + 4.3e-5 < 2^-12 of the exact one, relatively — still less than half an fp16 ulp (bf16: 2^-9), so its rounding is the
   reference's rounding or a neighbour of it.  The noise magnitude is 6..8 here (2..3 there): with scaling 0.3611 and sigma 0.35 the noise
   term must dominate the O(1) latents for the sum not to cancel.
   B = 2, (H, W) = (34, 58): 17 * 29 = 493 tokens per image, 986 lanes in four blocks of 256, the last one partial, and no token row ends on
   a wave boundary.  The output sits between guard elements, the inputs have NaN padding behind them.
 * an output that is not 16-byte aligned (the element-wise form of the same kernel);
 * at shift = 0, L = 4, fp16: the bits of gdf_op_vae_finish followed by torch's view / permute / reshape packing;
 * refusals (L = 17, odd H, odd W, null output) return an error and leave the output untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ops_binding import P, lib, ok, stream
from test_gpu_glue import _dominant, _signed, assert_owned, bits, gen, guard, is_guard, ord16, refused

pytestmark = pytest.mark.gpu

vp, ci, fp = C.c_void_p, C.c_int, C.c_float

B, H, W = 2, 34, 58
SHIFT, SCALING, SIGMA = 0.1159, 0.3611, 0.35
PAD = 104                      # guard elements on either side: 208 bytes, so the owned region starts 16-byte aligned (PAD_ODD: it does not)
PAD_ODD = 100

_CASES = [(L_, bf, q, en) for L_ in (4, 16) for bf in (0, 1) for q in (0, 1) for en in (0, 1)]


def plib():
    L = lib()
    L.gdf_op_vae_finish_packed.restype = ci
    L.gdf_op_vae_finish_packed.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, fp, fp, fp, fp, ci, vp, vp]
    return L


def f32(v):
    return float(np.float32(v))


def make_inputs(L_, use_wq, use_en, seed_extra=0):
    """test_vae_finish's recipe at (B, H * W); noise magnitude 6..8 (module docstring)"""
    g = gen(5000 + 100 * L_ + 8 * use_wq + 2 * use_en + seed_extra)
    L2, n = 2 * L_, B * H * W
    wq, sgn = _dominant(L2, g, L_) if use_wq else (None, torch.ones(L2))
    bq = torch.randn(L2, generator=g) * 0.05 if use_wq else None
    target = torch.empty(n, L2)
    target[:, :L_] = _signed((n, L_), 1.5, 2.5, g)
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])[torch.randint(0, 5, (n, L_), generator=g)]
    target[:, L_:] = lv + (torch.rand(n, L_, generator=g) - 0.5)
    h = target * sgn[None, :]
    eps = _signed((B, L_, H * W), 0.1, 0.3, g).half() if use_en else None
    noise = _signed((B, L_, H * W), 6.0, 8.0, g).half() if use_en else None
    return h, wq, bq, eps, noise


def pack_index(L_):
    """(L, H, W): position of latent (c, y, x) in one image's (S, 4L) token block"""
    c = torch.arange(L_).view(L_, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    return ((y // 2) * (W // 2) + x // 2) * (4 * L_) + c * 4 + (y % 2) * 2 + (x % 2)


def reference(L_, h, wq, bq, eps, noise, shift, scaling, na, nb):
    """float64 value and magnitude sum of every output, PACKED (B, S * 4L); asserts the premise of the 1-ulp bound on them"""
    h64 = h.double()
    if wq is not None:
        m = h64 @ wq.double().t() + bq.double()
        mabs = h64.abs() @ wq.double().abs().t() + bq.double().abs()
    else:
        m, mabs = h64, h64.abs()
    nchw = lambda t: t.reshape(B, H * W, L_).permute(0, 2, 1)
    z, zabs = nchw(m[:, :L_]) - f32(shift), nchw(mabs[:, :L_]) + abs(f32(shift))
    if eps is not None:
        sd = torch.exp(0.5 * nchw(m[:, L_:]).clamp(-30.0, 20.0)) * eps.double()
        z, zabs = z + sd, zabs + sd.abs()
    ref, mag = f32(scaling) * z, f32(scaling) * zabs
    if noise is not None:
        ref, mag = f32(na) * ref + f32(nb) * noise.double(), f32(na) * mag + f32(nb) * noise.double().abs()
    assert bool((ref.abs() * 8.0 >= mag).all()) and float(ref.abs().max()) < 60000.0       # the premise of the bound (test inputs, not the kernel)
    idx = pack_index(L_).reshape(-1)
    packed = torch.empty(B, L_ * H * W, dtype=torch.float64)
    packed[:, idx] = ref.reshape(B, -1)
    return packed


def padded(t):
    """the tensor on the device with 64 NaN elements behind it"""
    if t is None:
        return None
    flat = torch.cat([t.reshape(-1), torch.full((64,), float("nan"), dtype=t.dtype)]).cuda()
    return flat[:t.numel()]


def run(lb, L_, bf, h, wq, bq, eps, noise, shift, scaling, na, nb, pad=PAD):
    dt = torch.bfloat16 if bf else torch.float16
    n = B * L_ * H * W
    buf = guard((n + 2 * pad,), dt)
    out = buf[pad:pad + n]
    dev = [padded(t) for t in (h, wq, bq, eps, noise)]
    hd, wd, bd, ed, nd = dev
    ok(lb.gdf_op_vae_finish_packed(P(hd), B, H, W, L_, P(wd), P(bd), P(ed), P(nd), scaling, shift, na, nb, bf, P(out), stream()), lb)
    torch.cuda.synchronize()
    got = buf.cpu()
    owned = torch.zeros(buf.numel(), dtype=torch.bool)
    owned[pad:pad + n] = True
    assert_owned(got, owned)
    return got[pad:pad + n].reshape(B, -1), dev


def ulps(got, ref64):
    return (ord16(got) - ord16(ref64.to(got.dtype))).abs()


@pytest.mark.parametrize("L_,bf,use_wq,use_en", _CASES)
def test_vae_finish_packed(L_, bf, use_wq, use_en):
    lb = plib()
    h, wq, bq, eps, noise = make_inputs(L_, use_wq, use_en)
    na, nb = 1.0 - SIGMA, SIGMA
    ref = reference(L_, h, wq, bq, eps, noise, SHIFT, SCALING, na, nb)
    got, _ = run(lb, L_, bf, h, wq, bq, eps, noise, SHIFT, SCALING, na, nb)
    u = ulps(got, ref)
    print("vae_finish_packed L=%d bf16=%d wq=%d eps/noise=%d: max %d ulp, %.1f %% exact" % (L_, bf, use_wq, use_en, int(u.max()),
                                                                                           100.0 * float((u == 0).float().mean())))
    assert int(u.max()) <= 1


@pytest.mark.parametrize("L_,bf", [(16, 0), (6, 1), (5, 0)])
def test_vae_finish_packed_elementwise_form(L_, bf):
    """an output 8 bytes off a 16-byte boundary, an L no kernel is specialised for (6), an odd L (5): the element-wise accesses"""
    lb = plib()
    h, wq, bq, eps, noise = make_inputs(L_, 0, 1, seed_extra=1)
    na, nb = 1.0 - SIGMA, SIGMA
    ref = reference(L_, h, wq, bq, eps, noise, SHIFT, SCALING, na, nb)
    got, _ = run(lb, L_, bf, h, wq, bq, eps, noise, SHIFT, SCALING, na, nb, pad=PAD_ODD)
    assert int(ulps(got, ref).max()) <= 1
    if L_ == 6:                                              # and the same L on the aligned path: the same bits
        got2, _ = run(lb, L_, bf, h, wq, bq, eps, noise, SHIFT, SCALING, na, nb)
        assert bool((bits(got) == bits(got2)).all())


@pytest.mark.parametrize("use_wq", [0, 1])
def test_vae_finish_packed_equals_vae_finish_at_zero_shift(use_wq):
    """shift = 0, L = 4, fp16: gdf_op_vae_finish (in_scale = 1) followed by _pack_latents' view / permute / reshape, bit for bit"""
    lb, L_ = plib(), 4
    h, wq, bq, eps, noise = make_inputs(L_, use_wq, 1, seed_extra=2)
    na, nb = 1.0 - SIGMA, SIGMA
    got, (hd, wd, bd, ed, nd) = run(lb, L_, 0, h, wq, bq, eps, noise, 0.0, SCALING, na, nb)
    n = B * L_ * H * W
    one = guard((n + PAD,), torch.float16)
    ok(lb.gdf_op_vae_finish(P(hd), B, H * W, L_, P(wd), P(bd), P(ed), P(nd), SCALING, na, nb, 1.0, P(one), stream()), lb)
    torch.cuda.synchronize()
    nchw = one.cpu()[:n].view(B, L_, H, W)
    want = nchw.view(B, L_, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), L_ * 4)
    same = bits(got.reshape(want.shape)) == bits(want)
    assert bool(same.all()), "%d of %d elements differ from gdf_op_vae_finish + packing" % (int((~same).sum()), same.numel())


@pytest.mark.parametrize("L_,h_,w_,null_out", [(17, 34, 58, 0), (4, 33, 58, 0), (4, 34, 57, 0), (4, 34, 58, 1)])
def test_vae_finish_packed_refusals(L_, h_, w_, null_out):
    lb = plib()
    hm = torch.zeros(B * h_ * w_, 2 * L_, device="cuda")
    out = guard((B * L_ * h_ * w_ + 64,), torch.float16)
    rc = lb.gdf_op_vae_finish_packed(P(hm), B, h_, w_, L_, None, None, None, None, 1.0, 0.0, 1.0, 0.0, 0, None if null_out else P(out), stream())
    refused(lb, rc, "vae_finish_packed")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())
