"""The multi-timestep VAE tail and encode (-m gpu): gdf_op_vae_finish_multi (csrc/dit.hip vae_finish_multi_kernel) and gdf_vae_encode_multi
(csrc/vae.cpp) — the same B images noised for K timesteps from ONE pass over the moments / ONE encoder run, rows timestep-major (k * B + b).

 * the op against float64, in the manner of test_gpu_glue.py::test_vae_finish: the same input recipe (logvar crossing both clamp limits, no
   cancelling sums — asserted on the inputs) and the same bound, at most 1 fp16 ulp, which that test derives for this formula; the output sits
   between guard elements;
 * bit equality with the single-timestep kernel: K launches of gdf_op_vae_finish with the k-th scalars on the k-th eps / noise slices;
 * refusals leave the output untouched;
 * gdf_vae_encode_multi on one plan == K gdf_vae_encode calls on that plan, bit for bit: the tiny encoder, and the true SD VAE at 1024^2 with
   batch 8, the smallest case whose plan runs in sub-batches (chunk 4 < batch 8), i.e. whose tail writes rows k * B + c0 + j for c0 > 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ops_binding import P, lib, ok, stream
from test_gpu_glue import _dominant, _signed, assert_owned, bits, gen, guard, is_guard, refused, ulps16

pytestmark = pytest.mark.gpu

vp, ci, fp = C.c_void_p, C.c_int, C.c_float
FP = C.POINTER(C.c_float)


def mlib():
    L = lib()
    L.gdf_op_vae_finish_multi.restype = ci
    L.gdf_op_vae_finish_multi.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, fp, ci, FP, FP, FP, vp, vp]
    return L


def farr(v):
    return (C.c_float * len(v))(*v)


# K distinct coefficient triples (noise_a, noise_b, in_scale): a PNDM-like, an Euler-like and a third one
TRIPLES = [(0.8, 0.6, 0.75), (1.0, 1.7, 0.5), (0.35, 0.94, 1.0)]
PAD = 100

_FIN = [(L_, K, wq, bq, eps, noise) for L_ in (4, 8) for K in (1, 3) for wq, bq in ((0, 0), (1, 1), (1, 0)) for eps in (0, 1) for noise in (0, 1)]


def _inputs(L_, K, use_wq, use_bq, use_eps, use_noise, B, HW):
    """test_vae_finish's recipe, with eps / noise for K * B rows"""
    g = gen(1000 * K + 100 * L_ + 8 * use_wq + 4 * use_bq + 2 * use_eps + use_noise)
    L2 = 2 * L_
    wq, sgn = _dominant(L2, g, L_) if use_wq else (None, torch.ones(L2))
    bq = torch.randn(L2, generator=g) * 0.05 if use_bq else None
    target = torch.empty(B * HW, L2)
    target[:, :L_] = _signed((B * HW, L_), 1.5, 2.5, g)
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])[torch.randint(0, 5, (B * HW, L_), generator=g)]
    target[:, L_:] = lv + (torch.rand(B * HW, L_, generator=g) - 0.5)
    h = target * sgn[None, :]
    eps = _signed((K * B, L_, HW), 0.1, 0.3, g).half() if use_eps else None
    noise = _signed((K * B, L_, HW), 2.0, 3.0, g).half() if use_noise else None
    return h, wq, bq, eps, noise


def _run_multi(lb, h, wq, bq, eps, noise, B, HW, L_, K, scaling):
    """one launch into a buffer with PAD guard elements on either side -> the whole buffer on the CPU"""
    n = K * B * L_ * HW
    buf = guard((n + 2 * PAD,), torch.float16)
    out = buf[PAD:PAD + n]
    hd, wd, bd, ed, nd = [t.cuda() if t is not None else None for t in (h, wq, bq, eps, noise)]
    tr = TRIPLES[:K]
    ok(lb.gdf_op_vae_finish_multi(P(hd), B, HW, L_, P(wd), P(bd), P(ed), P(nd), scaling, K, farr([t[0] for t in tr]), farr([t[1] for t in tr]),
                                  farr([t[2] for t in tr]), P(out), stream()), lb)
    torch.cuda.synchronize()
    got = buf.cpu()
    owned = torch.zeros(buf.numel(), dtype=torch.bool)
    owned[PAD:PAD + n] = True
    assert_owned(got, owned)
    return got[PAD:PAD + n].reshape(K, B, L_, HW), (hd, wd, bd, ed, nd)


@pytest.mark.parametrize("L_,K,use_wq,use_bq,use_eps,use_noise", _FIN)
def test_vae_finish_multi(L_, K, use_wq, use_bq, use_eps, use_noise):
    """float64 reference, <= 1 fp16 ulp (the bound of test_gpu_glue.py::test_vae_finish: same formula, same inputs' premise); and bit equality
    with K launches of the single-timestep kernel.  B = 2, HW = 37 * 29: five blocks of 256 lanes for 2146 (image, pixel) pairs, the last partial."""
    lb, B, HW = mlib(), 2, 37 * 29
    scaling = 0.18215
    h, wq, bq, eps, noise = _inputs(L_, K, use_wq, use_bq, use_eps, use_noise, B, HW)
    got, (hd, wd, bd, ed, nd) = _run_multi(lb, h, wq, bq, eps, noise, B, HW, L_, K, scaling)

    f32 = lambda v: float(np.float32(v))
    h64 = h.double()
    if use_wq:
        m = h64 @ wq.double().t() + (bq.double() if use_bq else 0.0)
        mabs = h64.abs() @ wq.double().abs().t() + (bq.double().abs() if use_bq else 0.0)
    else:
        m, mabs = h64, h64.abs()
    nchw = lambda t: t.reshape(B, HW, L_).permute(0, 2, 1)
    worst = 0
    for k in range(K):
        na, nb, in_scale = TRIPLES[k]
        z, zabs = nchw(m[:, :L_]), nchw(mabs[:, :L_])
        if use_eps:
            sd = torch.exp(0.5 * nchw(m[:, L_:]).clamp(-30.0, 20.0)) * eps[k * B:(k + 1) * B].double()
            z, zabs = z + sd, zabs + sd.abs()
        ref, mag = f32(scaling) * z, f32(scaling) * zabs
        if use_noise:
            nk = noise[k * B:(k + 1) * B].double()
            ref, mag = f32(na) * ref + f32(nb) * nk, f32(na) * mag + f32(nb) * nk.abs()
        ref, mag = f32(in_scale) * ref, f32(in_scale) * mag
        assert bool((ref.abs() * 8.0 >= mag).all()) and float(ref.abs().max()) < 60000.0       # the premise of the bound (test inputs, not the kernel)
        u = ulps16(got[k], ref)
        worst = max(worst, int(u.max()))
        # the single-timestep kernel with the k-th scalars on the k-th slices: the same bits
        one = guard((B * L_ * HW + PAD,), torch.float16)
        ek = ed[k * B:(k + 1) * B] if ed is not None else None
        nk_ = nd[k * B:(k + 1) * B] if nd is not None else None
        ok(lb.gdf_op_vae_finish(P(hd), B, HW, L_, P(wd), P(bd), P(ek), P(nk_), scaling, na, nb, in_scale, P(one), stream()), lb)
        torch.cuda.synchronize()
        single = one.cpu()[:B * L_ * HW].reshape(B, L_, HW)
        assert bool((bits(single) == bits(got[k])).all()), "timestep %d: %d elements differ from gdf_op_vae_finish" % (
            k, int((bits(single) != bits(got[k])).sum()))
    print("vae_finish_multi L=%d K=%d wq=%d bq=%d eps=%d noise=%d: max %d ulp" % (L_, K, use_wq, use_bq, use_eps, use_noise, worst))
    assert worst <= 1
    if K > 1 and use_noise:
        assert not torch.equal(got[0], got[1])               # distinct triples and slices: the row blocks are not copies of each other


@pytest.mark.parametrize("n_t,L_", [(0, 4), (9, 4), (1, 9), (3, 9)])
def test_vae_finish_multi_refusals(n_t, L_):
    lb = mlib()
    h = torch.zeros(16, 2 * L_, device="cuda")
    out = guard((9 * 16 * 9 + 8,), torch.float16)
    c = farr([1.0] * 9)
    refused(lb, lb.gdf_op_vae_finish_multi(P(h), 1, 16, L_, None, None, None, None, 1.0, n_t, c, c, c, P(out), stream()), "vae_finish_multi")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


def _encode_multi_equals_singles(enc, image, B, K, lat, sf):
    g = torch.Generator().manual_seed(7)
    eps = torch.randn(K * B, 4, lat, lat, generator=g).half().cuda()
    noise = torch.randn(K * B, 4, lat, lat, generator=g).half().cuda()
    coef = [(0.95, 0.31, 1.0), (1.0, 0.7, 0.82)][:K]
    singles = []
    for k, (a, b, s) in enumerate(coef):
        singles.append(enc.encode(image, eps=eps[k * B:(k + 1) * B], noise=noise[k * B:(k + 1) * B], scaling_factor=sf, noise_a=a, noise_b=b,
                                  input_scale=s).clone())
    for rep in range(2):                                  # (the second call of a binding replays the graph the first one left)
        multi = enc.encode_multi(image, eps=eps, noise=noise, scaling_factor=sf, noise_a=[c[0] for c in coef], noise_b=[c[1] for c in coef],
                                 input_scale=[c[2] for c in coef]).clone()
        torch.cuda.synchronize()
        assert tuple(multi.shape) == (K * B, 4, lat, lat) and multi.dtype == torch.float16
        assert torch.isfinite(multi.float()).all()
        for k in range(K):
            assert torch.equal(multi[k * B:(k + 1) * B], singles[k]), (rep, k)
    assert not torch.equal(multi[:B], multi[B:2 * B])
    # and the single call after the multi one, on the same plan and hook-buffer pool: still its own bits
    a, b, s = coef[0]
    again = enc.encode(image, eps=eps[:B], noise=noise[:B], scaling_factor=sf, noise_a=a, noise_b=b, input_scale=s)
    assert torch.equal(again, singles[0])
    assert len(enc._plans) == 1                           # one plan (and one workspace) served every call above
    # posterior mode without noise: eps / noise NULL on the multi path
    mode = enc.encode_multi(image, eps=None, noise=None, scaling_factor=sf, noise_a=[1.0] * K, noise_b=[0.0] * K, input_scale=[1.0, 0.5][:K])
    ref = enc.encode(image, eps=None, noise=None, scaling_factor=sf, noise_a=1.0, noise_b=0.0, input_scale=1.0)
    assert torch.equal(mode[:B], ref)


def test_vae_encode_multi_tiny():
    """the tiny 4-level encoder of test_gpu_vae.py, B = 3, K = 2"""
    from components.native import NativeVAEEncoder
    from oracle import vae_ref as VR
    channels, img, B, K = (64, 128, 256, 256), 128, 3, 2
    arch = VR.tiny_arch(channels)
    Pm = VR.synth_params(arch, seed=0)
    image = (torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(1)) * 2 - 1).half().cuda()
    enc = NativeVAEEncoder(dict(in_channels=3, latent_channels=4, block_out_channels=channels, layers_per_block=2, use_quant_conv=1), device="cuda:0")
    enc.load_vae_state_dict({k: v.half() for k, v in Pm.items()})
    assert enc.ready()
    _encode_multi_equals_singles(enc, image, B, K, img >> 3, 0.18215)
    with pytest.raises(ValueError):
        enc.encode_multi(image, noise_a=[1.0] * 9, noise_b=[0.0] * 9, input_scale=[1.0] * 9)
    with pytest.raises(ValueError):
        enc.encode_multi(image, noise_a=[], noise_b=[], input_scale=[])


def test_vae_encode_multi_full_size_sub_batches():
    """The true SD VAE at 1024^2, batch 8: the widest activation is 2^28 bytes per image, 8 of them are not below 2^31, so the plan runs two
    passes of 4 images — the only way to reach the tail's row arithmetic k * B + c0 + j with c0 > 0.  K = 2."""
    from components.native import VAE_CONFIGS, NativeVAEEncoder
    B, K, img = 8, 2, 1024
    enc = NativeVAEEncoder(VAE_CONFIGS["sd"], device="cuda:0")
    enc.init_synthetic(3)
    assert enc.ready()
    image = (torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(2)) * 2 - 1).half().cuda()
    _encode_multi_equals_singles(enc, image, B, K, img >> 3, 0.13025)
