"""Kernel-level parity (-m gpu) of the glue kernels of csrc/norm.hip, csrc/dit.hip and csrc/post.hip through the C ABI (include/gdf_ops.h):
embedding / packing kernels, the VAE head and tail, the patch layouts, the load-time weight re-layouts and the output-stage post-processing.

Every case compares ONE launch with a plain CPU reference (float64 arithmetic, or integer indexing for the byte movers) on inputs drawn from a
seeded generator.  Results are bit-exact unless a bound is stated; every stated bound is derived from the number formats (see each test), none
is a measured figure.  Every destination is allocated larger than the op needs and pre-filled with a NaN bit pattern (`guard`): each test
asserts that everything the op owns was written and that pad columns, rows past the end and foreign channels still hold the pattern, so an
off-by-one in a grid-stride bound shows as a changed guard element, not as a fault.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ops_binding import P, lib, ok, stream, vp

pytestmark = pytest.mark.gpu

PAT16, PAT32 = 0x7FDA, 0x7FC0A5A5          # NaN in fp16, bf16 / fp32, with a payload no kernel produces


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def guard(shape, dtype, device="cuda"):
    """a tensor whose every element holds the guard pattern"""
    if dtype == torch.float32:
        return torch.full(shape, PAT32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full(shape, PAT16, dtype=torch.int16, device=device).view(dtype)


def is_guard(t):
    return bits(t) == (PAT32 if t.element_size() == 4 else PAT16)


def assert_bits(got, want):
    """`want` was built on the CPU from a guard tensor: equal bits = all owned elements right AND every other element untouched"""
    got = got.cpu()
    same = bits(got) == bits(want)
    assert bool(same.all()), "%d of %d elements differ, first at flat index %d" % (
        int((~same).sum()), same.numel(), int((~same).flatten().nonzero()[0]))


def assert_owned(got_cpu, owned):
    """toleranced cases: the owned region holds no guard element, everything else only guard elements"""
    g = is_guard(got_cpu)
    assert not bool(g[owned].any()), "%d owned elements were not written" % int(g[owned].sum())
    assert bool(g[~owned].all()), "%d elements outside the op's region were written" % int((~g[~owned]).sum())


def ord16(t):
    """fp16 bits as integers ordered like the values (+-0 -> 0): differences count ulps"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulps16(got, ref64):
    """distance in fp16 ulps between an fp16 tensor and the fp16 rounding of a float64 reference"""
    return (ord16(got) - ord16(ref64.to(torch.float16))).abs()


def refused(L, rc, name):
    assert rc != 0
    assert name in L.gdf_last_error().decode(), L.gdf_last_error().decode()


def finite16(n, dtype, seed):
    """n random 16-bit patterns of `dtype` (fp16 / bf16) covering every exponent incl. subnormals, without inf / NaN, plus the edge values"""
    b = torch.randint(-32768, 32768, (n,), generator=gen(seed), dtype=torch.int32)
    emask = 0x7C00 if dtype == torch.float16 else 0x7F80
    b = torch.where((b & emask) == emask, b & ~0x0400 & ~0x0080, b)                  # all-ones exponent -> a finite neighbour
    edge = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF] if dtype == torch.float16 else \
           [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x477F]
    b[:len(edge)] = torch.tensor(edge, dtype=torch.int32)
    b = torch.where(b >= 32768, b - 65536, b)
    return b.to(torch.int16).view(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# embedding and vector kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _ulp16_of(x):
    """fp16 ulp at magnitude x (float64 tensor), subnormal range included"""
    e = torch.floor(torch.log2(x.clamp_min(2.0 ** -24))).clamp_min(-14.0)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10.0)


@pytest.mark.parametrize("round_f16", [0, 1])
@pytest.mark.parametrize("tscale", [1.0, 1000.0])
@pytest.mark.parametrize("n_per_row", [1, 6])
@pytest.mark.parametrize("dim", [256, 320])
def test_sinusoid(dim, n_per_row, tscale, round_f16):
    """get_timestep_embedding, [cos | sin].  Bound per element: 2^-21 |arg| + 2^-22 — the three fp32 roundings of the argument (t * tscale,
    the frequency's exponent, the product: 3 * 2^-24 |arg|) and <= 2 ulp of expf on the frequency (2^-22 |arg|) move the argument by
    < 2^-21 |arg|, which moves cos / sin by no more; <= 2 ulp of sinf / cosf on a value <= 1 and the store add 2^-22.  round_f16 adds
    half an fp16 ulp of the value.  The frequency itself must be rounded once for this to hold: its exponent -ln(10000) f / half, of magnitude up
    to 9.2, evaluated in fp32 would alone cost 2^-19.5 |arg|."""
    L, B = lib(), 3
    col_off = 40 if n_per_row > 1 else 0                     # the SDXL time_ids form writes behind the pooled text embedding
    ldo = col_off + n_per_row * dim + 24
    tsets = [[0.0, 1.0, 999.0], [0.5, 999.0, 1.0]] if n_per_row == 1 else \
            [[0.0, 1.0, 999.0, 0.5, 1024.0, 37.25, 999.0, 0.5, 0.0, 1.0, 512.0, 3.0, 0.5, 0.0, 1.0, 999.0, 768.0, 64.0]]
    for ts in tsets:
        t = torch.tensor(ts, dtype=torch.float32).reshape(B, n_per_row)
        out = guard((B + 1, ldo), torch.float32)
        td = t.cuda()
        ok(L.gdf_op_sinusoid(P(td), B, n_per_row, dim, P(out), ldo, col_off, round_f16, tscale, stream()), L)
        torch.cuda.synchronize()
        got = out.cpu()
        owned = torch.zeros(B + 1, ldo, dtype=torch.bool)
        owned[:B, col_off:col_off + n_per_row * dim] = True
        assert_owned(got, owned)                             # columns [0, col_off) and [col_off + n dim, ldo) and row B keep the guard
        half = dim // 2
        f = torch.arange(half, dtype=torch.float64)
        arg = (t.double() * tscale)[:, :, None] * torch.exp(-math.log(10000.0) * f / half)[None, None, :]       # [B][n][half]
        ref = torch.cat([torch.cos(arg), torch.sin(arg)], dim=2).reshape(B, n_per_row * dim)
        bound = (2.0 ** -21 * arg.abs() + 2.0 ** -22).repeat(1, 1, 2).reshape(B, n_per_row * dim)
        if round_f16:
            bound = bound + 0.5 * _ulp16_of(ref.abs() + bound)
        err = (got[:B, col_off:col_off + n_per_row * dim].double() - ref).abs()
        print("sinusoid dim=%d n=%d tscale=%g f16=%d: max err %.3e, max err / bound %.3f" % (dim, n_per_row, tscale, round_f16, float(err.max()),
                                                                                           float((err / bound).max())))
        assert bool((err <= bound).all()), "max err / bound = %.3f" % float((err / bound).max())


@pytest.mark.parametrize("n", [1280, 2047])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_widen(dtype, n):
    L, B, col_off = lib(), 3, 24
    ldo = col_off + n + 9
    x = finite16(B * n, dtype, seed=n).reshape(B, n)
    out = guard((B + 1, ldo), torch.float32)
    xd = x.cuda()
    ok(L.gdf_op_widen(P(xd), int(dtype == torch.bfloat16), B, n, P(out), ldo, col_off, stream()), L)
    torch.cuda.synchronize()
    want = guard((B + 1, ldo), torch.float32, "cpu")
    want[:B, col_off:col_off + n] = x.float()                # exact: every fp16 / bf16 value (subnormals, +-0, +-max) is an fp32 value
    assert_bits(out, want)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_silu_vec(n):
    """|got - silu(x)| <= 2^-21 |silu(x)| + 2^-126: expf (<= 2 ulp), the add and the division round three times, 2^-22 + 2 * 2^-24 < 2^-21;
    the floor is the smallest normal number (results below it have fewer bits).  Where expf(-x) overflows (x < -88.7) the quotient must
    still be a number: silu(-90) = -7.4e-38."""
    L = lib()
    x = (torch.rand(n, generator=gen(n), dtype=torch.float64) * 180.0 - 90.0).float()
    special = torch.tensor([-90.0, -89.0, -88.75, -88.5, -88.0, -87.5, -0.0, 0.0, 90.0, 88.8, -20.0, 1.0], dtype=torch.float32)
    k = min(n, special.numel())
    x[n - k:] = special[:k]                                    # (n = 1: -90)
    out = guard((n + 64,), torch.float32)
    xd = x.cuda()
    ok(L.gdf_op_silu_vec(P(xd), P(out), n, stream()), L)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(n + 64, dtype=torch.bool)
    owned[:n] = True
    assert_owned(got, owned)
    assert not bool(torch.isnan(got[:n]).any())
    xr = x.double()
    ref = xr / (1.0 + torch.exp(-xr))
    err = (got[:n].double() - ref).abs()
    bound = 2.0 ** -21 * ref.abs() + 2.0 ** -126
    print("silu_vec n=%d: max err / bound %.3f" % (n, float((err / bound).max())))
    assert bool((err <= bound).all()), "x = %r: err / bound = %.3f" % (float(x[(err / bound).argmax()]), float((err / bound).max()))


@pytest.mark.parametrize("period", [6 * 1152, 1152])
def test_add_table(period):
    L, B, n = lib(), 3, 6 * 1152
    ldvec, ldo = period + 8, n + 16
    g = gen(period)
    table = torch.randn(n, generator=g)
    vec = torch.randn(B, ldvec, generator=g)
    out = guard((B + 1, ldo), torch.float32)
    td, vd = table.cuda(), vec.cuda()
    ok(L.gdf_op_add_table(P(td), P(vd), ldvec, period, B, n, P(out), ldo, stream()), L)
    torch.cuda.synchronize()
    want = guard((B + 1, ldo), torch.float32, "cpu")
    want[:B, :n] = table[None, :] + vec[:, :period].repeat(1, n // period)          # one fp32 addition per element: bit-exact
    assert_bits(out, want)


def _small_linear(L, x, W, bias, N, silu_in, out, ldo):
    M, K = x.shape
    xd, wd, bd = x.cuda(), W.cuda(), bias.cuda()
    ok(L.gdf_op_small_linear_ex(P(xd), K, M, K, P(wd), int(W.dtype == torch.bfloat16), P(bd), N, silu_in, 0, P(out), ldo, stream()), L)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("N", [1000, 4096])                   # the column-per-wave kernel / the LDS-staged wide kernel (N >= 1024)
def test_small_linear_bf16_weights(N):
    """bf16 weights, bit-exact: x are multiples of 2^-3 in [-4, 4], W multiples of 2^-6 in [-2, 2] (bf16 values), the bias multiples of 2^-9:
    every product and every partial sum is a multiple of 2^-9 below 2^12, i.e. exact in fp32 in ANY summation order — the float64 sum is
    the only right answer, whatever the lane split and the reduction tree."""
    L, M, K = lib(), 5, 328                                   # K % 512 != 0: the last lanes of a wave run out of columns first
    g = gen(N)
    x = torch.randint(-32, 33, (M, K), generator=g).float() / 8.0
    W = (torch.randint(-128, 129, (N, K), generator=g).float() / 64.0).to(torch.bfloat16)
    assert torch.equal(W.float() * 64.0, (W.float() * 64.0).round())
    bias = torch.randint(-512, 513, (N,), generator=g).float() / 512.0
    ldo = N + 8
    got = _small_linear(L, x, W, bias, N, 0, guard((M + 1, ldo), torch.float32), ldo)
    want = guard((M + 1, ldo), torch.float32, "cpu")
    want[:M, :N] = (x.double() @ W.double().t() + bias.double()).float()
    assert_bits(got, want)


@pytest.mark.parametrize("M", [8, 12])
@pytest.mark.parametrize("N", [1000, 4096])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_small_linear_identical_rows_get_identical_bits(dtype, N, M):
    """M copies of one input row (a batch of identical samples): every output row must carry the same bits, in both kernels and in the second
    launch of the wide one (rows 8..11).  The values themselves: |got - ref| <= (K + 8) 2^-24 (|bias| + sum_k |silu(x_k) W_k|): K roundings
    of the running sum at worst, and 2^-21 = 8 * 2^-24 for the relative error of each silu (test_silu_vec)."""
    L, K = lib(), 328
    g = gen(N + M)
    row = torch.randn(K, generator=g) * 2.0
    x = row[None, :].repeat(M, 1).contiguous()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    ldo = N + 8
    got = _small_linear(L, x, W, bias, N, 1, guard((M + 1, ldo), torch.float32), ldo)
    owned = torch.zeros(M + 1, ldo, dtype=torch.bool)
    owned[:M, :N] = True
    assert_owned(got, owned)
    for m in range(1, M):
        assert torch.equal(bits(got[m, :N]), bits(got[0, :N])), "row %d differs from row 0" % m
    s = row.double() / (1.0 + torch.exp(-row.double()))
    ref = W.double() @ s + bias.double()
    mag = W.double().abs() @ s.abs() + bias.double().abs()
    assert bool(((got[0, :N].double() - ref).abs() <= (K + 8) * 2.0 ** -24 * mag).all())


# ------------------------------------------------------------------------------------------------------------------------------
# layout kernels: bit-exact against integer indexing
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,hook", [(2, 7, 9, 4, 0), (2, 7, 9, 4, 1), (2, 7, 9, 8, 0), (2, 7, 9, 8, 1),
                                            (5, 512, 512, 4, 1)])      # 1.3 M pixels > 4096 * 256: the stride loop runs twice
def test_pack_latents(B, H, W, Cin, hook):
    L = lib()
    x = torch.randn(B, Cin, H, W, generator=gen(Cin)).half()
    x[x == 0] = 1.0                                           # a zero in channels [Cin, 8) is then a written zero
    n = B * H * W
    o8 = guard((n + 3, 8), torch.float16)
    hk = guard((n + 3, Cin), torch.float16) if hook else None
    xd = x.cuda()
    ok(L.gdf_op_pack_latents(P(xd), B, Cin, H, W, P(o8), P(hk), stream()), L)
    torch.cuda.synchronize()
    nhwc = x.permute(0, 2, 3, 1).reshape(n, Cin)
    want = guard((n + 3, 8), torch.float16, "cpu")
    want[:n] = 0.0
    want[:n, :Cin] = nhwc
    assert_bits(o8, want)
    if hook:
        wh = guard((n + 3, Cin), torch.float16, "cpu")
        wh[:n] = nhwc
        assert_bits(hk, wh)


def test_pack_latents_refuses_more_than_8_channels():
    L = lib()
    x = torch.zeros(1, 9, 4, 4, dtype=torch.half, device="cuda")
    o8 = guard((16, 8), torch.float16)
    refused(L, L.gdf_op_pack_latents(P(x), 1, 9, 4, 4, P(o8), None, stream()), "pack_latents")
    torch.cuda.synchronize()
    assert bool(is_guard(o8.cpu()).all())


def _patch_rows(x, p):
    """column (c * p + py) * p + px of row (b, ty, tx): the Conv2d weight order"""
    B, Cc, H, W = x.shape
    return x.reshape(B, Cc, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), Cc * p * p)


@pytest.mark.parametrize("p,Cin,kpad", [(2, 4, 64), (1, 4, 64), (1, 8, 8)])
def test_patchify(p, Cin, kpad):
    L, B, H, W = lib(), 2, 12, 20
    x = torch.randn(B, Cin, H, W, generator=gen(p)).half()
    x[x == 0] = 1.0
    rows = B * (H // p) * (W // p)
    out = guard((rows + 2, kpad), torch.float16)
    xd = x.cuda()
    ok(L.gdf_op_patchify(P(xd), B, Cin, H, W, p, kpad, P(out), stream()), L)
    torch.cuda.synchronize()
    want = guard((rows + 2, kpad), torch.float16, "cpu")
    want[:rows] = 0.0
    want[:rows, :Cin * p * p] = _patch_rows(x, p)
    assert_bits(out, want)


def _unpatch(tok, B, Cout, gh, gw, p):
    """'nhwpqc -> nchpwq'"""
    return tok.reshape(B, gh, gw, p, p, Cout).permute(0, 5, 1, 3, 2, 4).reshape(B, Cout, gh * p, gw * p)


@pytest.mark.parametrize("p", [2, 1])
def test_unpatchify(p):
    L, B, Cout, H, W = lib(), 2, 8, 12, 20
    gh, gw = H // p, W // p
    tok = torch.randn(B * gh * gw, p * p * Cout, generator=gen(10 + p)).half()
    n = B * Cout * H * W
    out = guard((n + 300,), torch.float16)
    td = tok.cuda()
    ok(L.gdf_op_unpatchify(P(td), B, Cout, gh, gw, p, P(out), stream()), L)
    torch.cuda.synchronize()
    want = guard((n + 300,), torch.float16, "cpu")
    want[:n] = _unpatch(tok, B, Cout, gh, gw, p).reshape(-1)
    assert_bits(out, want)


@pytest.mark.parametrize("p,Cc", [(1, 8), (2, 1)])            # the two column orders coincide when p = 1 or there is one channel
def test_unpatchify_inverts_patchify(p, Cc):
    L, B, H, W = lib(), 2, 12, 20
    x = torch.randn(B, Cc, H, W, generator=gen(20 + p)).half()
    kpad = Cc * p * p                                         # token width = p * p * Cout: no padding between the two kernels
    xd = x.cuda()
    tok = guard((B * (H // p) * (W // p) + 1, kpad), torch.float16)
    back = guard((x.numel() + 64,), torch.float16)
    ok(L.gdf_op_patchify(P(xd), B, Cc, H, W, p, kpad, P(tok), stream()), L)
    ok(L.gdf_op_unpatchify(P(tok), B, Cc, H // p, W // p, p, P(back), stream()), L)
    torch.cuda.synchronize()
    want = guard((x.numel() + 64,), torch.float16, "cpu")
    want[:x.numel()] = x.reshape(-1)
    assert_bits(back, want)


def test_patchify_refusals():
    L = lib()
    x = torch.zeros(1, 4, 13, 20, dtype=torch.half, device="cuda")
    out = guard((256, 64), torch.float16)
    refused(L, L.gdf_op_patchify(P(x), 1, 4, 13, 20, 2, 64, P(out), stream()), "patchify")        # H % p != 0
    refused(L, L.gdf_op_patchify(P(x), 1, 4, 12, 20, 2, 8, P(out), stream()), "patchify")         # Cin * p * p = 16 > kpad
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


def _src(shape, code, seed):
    """a weight tensor in source dtype `code` (0 fp16, 1 fp32, 2 bf16) and its fp32 values"""
    w = torch.randn(*shape, generator=gen(seed))
    w = w.half() if code == 0 else w.to(torch.bfloat16) if code == 2 else w
    return w, w.float()


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("R,ksrc,kdst", [(1152, 16, 64), (5, 70, 128)])
def test_relayout_rows_padk(R, ksrc, kdst, f32):
    L = lib()
    wf = torch.randn(R, ksrc, generator=gen(R))
    wf[wf.half() == 0] = 1.0                                  # a zero in the pad columns is then a written zero
    w = wf if f32 else wf.half()
    wf = w.float()
    dst = guard((R + 1, kdst), torch.float16)
    wd = w.cuda()
    ok(L.gdf_op_relayout_rows_padk(P(wd), f32, P(dst), R, ksrc, kdst, stream()), L)
    torch.cuda.synchronize()
    want = guard((R + 1, kdst), torch.float16, "cpu")
    want[:R] = 0.0
    want[:R, :ksrc] = wf.half()                               # fp32 -> fp16: round to nearest even on both sides
    assert_bits(dst, want)


def _conv_layout(wf, ipad, tpad, cblk):
    O, I, T = wf.shape
    pad = torch.zeros(O, ipad, tpad)
    pad[:, :I, :T] = wf
    if cblk:
        return pad.reshape(O, ipad // cblk, cblk, tpad).permute(0, 1, 3, 2).reshape(-1).half()    # [o][i / cblk][t][i % cblk]
    return pad.permute(0, 2, 1).reshape(-1).half()                                               # [o][t][i]


@pytest.mark.parametrize("O,I,T,ipad,tpad,cblk,code", [
    (5, 70, 1, 128, 2, 0, 0), (5, 70, 4, 128, 6, 0, 1), (5, 70, 9, 128, 16, 0, 2), (5, 70, 9, 128, 9, 0, 1),
    (5, 70, 9, 128, 9, 64, 0), (5, 70, 9, 128, 16, 64, 2), (5, 70, 4, 128, 4, 64, 1),
    (1100, 70, 9, 128, 16, 0, 0), (1100, 70, 9, 128, 16, 64, 1)])      # 2.25 M elements > 8192 * 256: the stride loop runs twice
def test_relayout_conv(O, I, T, ipad, tpad, cblk, code):
    L = lib()
    w, wf = _src((O, I, T), code, seed=T + cblk)
    n = O * ipad * tpad
    dst = guard((n + 512,), torch.float16)
    wd = w.cuda()
    ok(L.gdf_op_relayout_conv(P(wd), code, P(dst), O, I, T, ipad, tpad, cblk, stream()), L)
    torch.cuda.synchronize()
    want = guard((n + 512,), torch.float16, "cpu")
    want[:n] = _conv_layout(wf, ipad, tpad, cblk)
    assert_bits(dst, want)


def test_relayout_conv_refuses_ipad_not_a_multiple_of_cblk():
    L = lib()
    w = torch.zeros(2, 70, 9, dtype=torch.half, device="cuda")
    dst = guard((2 * 100 * 9 + 64,), torch.float16)
    refused(L, L.gdf_op_relayout_conv(P(w), 0, P(dst), 2, 70, 9, 100, 9, 64, stream()), "relayout_conv")
    torch.cuda.synchronize()
    assert bool(is_guard(dst.cpu()).all())


def _geglu_rows(R, g):
    """destination row of source row r of a [h rows | gate rows] matrix: every 2g rows are [g h | g gate]"""
    half = R // 2
    r = torch.arange(R)
    gate = r >= half
    rr = torch.where(gate, r - half, r)
    return (rr // g) * 2 * g + gate.long() * g + rr % g


def _ties_bf16(shape, seed):
    """fp32 values of which half lie exactly between two bf16 neighbours (even and odd ones): round-to-nearest-even shows"""
    w = torch.randn(*shape, generator=gen(seed))
    b = w.view(torch.int32).clone()
    tie = torch.rand(*shape, generator=gen(seed + 1)) < 0.5
    b = torch.where(tie, (b & ~0xFFFF) | 0x8000, b)
    return b.view(torch.float32)


@pytest.mark.parametrize("case", ["identity_off", "geglu", "bf16_dst", "bf16_dst_geglu", "large"])
def test_relayout_rows(case):
    L = lib()
    R, K, off, g, code, dbf = {"identity_off": (37, 24, 5, 0, 0, 0), "geglu": (96, 24, 0, 16, 2, 0), "bf16_dst": (37, 24, 3, 0, 1, 1),
                               "bf16_dst_geglu": (96, 40, 0, 16, 1, 1), "large": (2100, 1000, 2, 0, 0, 0)}[case]
    if dbf:
        wf = _ties_bf16((R, K), seed=7)
        w = wf
    else:
        w, wf = _src((R, K), code, seed=R)
    ddt = torch.bfloat16 if dbf else torch.float16
    rows = R + off + 4                                        # the block sits at rows [off, off + R) of a larger (stacked) matrix
    dst = guard((rows, K), ddt)
    wd = w.cuda()
    ok(L.gdf_op_relayout_rows(P(wd), code, P(dst), R, K, off, g, dbf, stream()), L)
    torch.cuda.synchronize()
    want = guard((rows, K), ddt, "cpu")
    dr = _geglu_rows(R, g) if g else torch.arange(R) + off
    want[dr] = wf.to(ddt)                                     # CPU casts round to nearest even
    assert_bits(dst, want)


@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("R,off,g", [(300, 7, 0), (320, 0, 16)])          # more than one block of 256
def test_relayout_vec(R, off, g, code):
    L = lib()
    w, wf = _src((R,), code, seed=R + code)
    dst = guard((R + off + 9,), torch.float32)
    wd = w.cuda()
    ok(L.gdf_op_relayout_vec(P(wd), code, P(dst), R, off, g, stream()), L)
    torch.cuda.synchronize()
    want = guard((R + off + 9,), torch.float32, "cpu")
    want[_geglu_rows(R, g) if g else torch.arange(R) + off] = wf
    assert_bits(dst, want)


# ---- copy2d_kernel<true>: the hook store of the MMDiT path ----
def _split(x32, dtype=torch.float16):
    hi = x32.to(dtype)
    lo = (x32 - hi.float()).to(dtype)
    return hi, lo


def _copy2d_ex(L, s16, s32, lds, R, Cc, bf, sat, s_lo, scale, ldd):
    dst = guard((R + 1, ldd), torch.float16)
    a, b = (s16.cuda() if s16 is not None else None), (s32.cuda() if s32 is not None else None)
    ok(L.gdf_op_copy2d_ex(P(a), P(b), lds, P(dst), ldd, R, Cc, bf, sat, s_lo, scale, stream()), L)
    torch.cuda.synchronize()
    return dst.cpu()


def _copy_want(R, Cc, ldd, val16):
    want = guard((R + 1, ldd), torch.float16, "cpu")
    want[:R, :Cc] = val16
    return want


@pytest.mark.parametrize("Cc", [40, 37])                      # 40 with lds, ldd % 8 == 0: 16-byte lanes; 37: one element per lane
def test_copy2d_ex_forms(Cc):
    L, R, lds, ldd, s_lo = lib(), 50, 96, 56, 48
    g = gen(Cc)
    # bf16 source -> fp16
    s = (torch.randn(R, lds, generator=g) * 8.0).to(torch.bfloat16)
    assert_bits(_copy2d_ex(L, s, None, lds, R, Cc, 1, 0, 0, 1.0, ldd), _copy_want(R, Cc, ldd, s[:, :Cc].float().half()))
    # split-pair sources: dst = fp16(fp32(hi) + fp32(lo))
    x32 = torch.randn(R, Cc, generator=g) * 8.0
    for dt in (torch.float16, torch.bfloat16):
        hi, lo = _split(x32, dt)
        s = torch.zeros(R, lds, dtype=dt)
        s[:, :Cc], s[:, s_lo:s_lo + Cc] = hi, lo
        got = _copy2d_ex(L, s, None, lds, R, Cc, int(dt == torch.bfloat16), 0, s_lo, 1.0, ldd)
        assert_bits(got, _copy_want(R, Cc, ldd, (hi.float() + lo.float()).half()))
    # scale: dst = fp16(scale * src), one fp32 product
    s = torch.randn(R, lds, generator=g).half()
    assert_bits(_copy2d_ex(L, s, None, lds, R, Cc, 0, 0, 0, 0.125, ldd), _copy_want(R, Cc, ldd, (s[:, :Cc].float() * 0.125).half()))
    s32 = torch.randn(R, lds, generator=g) * 100.0
    assert_bits(_copy2d_ex(L, None, s32, lds, R, Cc, 0, 0, 0, 1.5, ldd), _copy_want(R, Cc, ldd, (s32[:, :Cc] * 1.5).half()))


@pytest.mark.parametrize("Cc", [40, 37])
def test_copy2d_ex_saturates(Cc):
    """sat = 1: values beyond the fp16 range store +-65504 and a NaN stays a NaN; sat = 0: the same values store +-inf"""
    L, R, lds, ldd = lib(), 50, 96, 56
    s32 = torch.randn(R, lds, generator=gen(Cc)) * 3.0e4                             # about a third beyond +-65504 after the edits below
    s32[0, :8] = torch.tensor([65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1.0e30, -1.0e30, 7.0e4])
    s32[1, :4] = torch.tensor([float("inf"), float("-inf"), 3.0e38, -3.0e38])
    s32[::7, 5] *= 4.0
    nan_at = torch.zeros(R, Cc, dtype=torch.bool)
    nan_at[2, 3] = nan_at[9, Cc - 1] = nan_at[R - 1, 0] = True
    s32[:, :Cc][nan_at] = float("nan")
    assert int((s32[:, :Cc].abs() > 65504).sum()) > 20
    for sat in (1, 0):
        got = _copy2d_ex(L, None, s32, lds, R, Cc, 0, sat, 0, 1.0, ldd)
        owned = torch.zeros(R + 1, ldd, dtype=torch.bool)
        owned[:R, :Cc] = True
        assert_owned(got, owned)
        v = got[:R, :Cc]
        assert bool(torch.isnan(v[nan_at]).all()), "a NaN did not stay a NaN (sat = %d): %r" % (sat, v[nan_at].tolist())
        ref = (s32[:, :Cc].clamp(-65504.0, 65504.0) if sat else s32[:, :Cc]).half()
        assert torch.equal(bits(v[~nan_at]), bits(ref[~nan_at]))
        if sat:
            assert not bool(torch.isinf(v).any())
        else:
            assert bool(torch.isinf(v[s32[:, :Cc].abs() >= 65520.0]).all())
    # the 16-bit sources saturate too: bf16 values beyond the fp16 range
    s = (torch.randn(R, lds, generator=gen(Cc + 1)) * 6.0e4).to(torch.bfloat16)
    got = _copy2d_ex(L, s, None, lds, R, Cc, 1, 1, 0, 1.0, ldd)
    assert_bits(got, _copy_want(R, Cc, ldd, s[:, :Cc].float().clamp(-65504.0, 65504.0).half()))


def test_copy2d_ex_stride_loop():
    """R * C / 8 = 1.05 M lanes of work > 4096 * 256: every lane of the 16-byte path takes a second trip"""
    L, R, Cc = lib(), 2100, 4000
    s = (torch.randn(R, Cc, generator=gen(3)) * 3.0e4).to(torch.bfloat16)
    got = _copy2d_ex(L, s, None, Cc, R, Cc, 1, 1, 0, 0.5, Cc + 8)
    assert_bits(got, _copy_want(R, Cc, Cc + 8, (s.float() * 0.5).clamp(-65504.0, 65504.0).half()))


# ------------------------------------------------------------------------------------------------------------------------------
# VAE head and tail.  Bound: within 1 fp16 ulp of the fp16-rounded float64 reference.  The kernels evaluate fp32 dot products of <= 16 terms
# and a handful of fp32 operations, then round once.  The inputs below are built so that no sum cancels: every output is at least 1/8 of
# the sum of the magnitudes of its terms (asserted on the float64 side).  The fp32 value is then within
# 8 * (16 + 8) * 2^-24 + (error of exp: 0.5 * 2^-14.6 from its argument, a <= 16-term sum of magnitude <= 45, + 2 ulp) < 2^-12 of the exact
# one, relatively: less than half an fp16 ulp, so its rounding is the reference's rounding or a neighbour of it.
# ------------------------------------------------------------------------------------------------------------------------------
def _dominant(n, g, small_from=None):
    """[n][n] fp16 weights: +-1 on the diagonal, N(0, 0.01) elsewhere (N(0, 0.001) in the columns from `small_from` up, whose inputs are
    20 times larger); and the diagonal's signs"""
    sgn = torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0
    w = (torch.randn(n, n, generator=g) * 0.01)
    if small_from is not None:
        w[:, small_from:] *= 0.1
    w[torch.arange(n), torch.arange(n)] = sgn
    return w.half(), sgn


def _signed(shape, lo, hi, g):
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo) * (torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0)


_FIN = [(L_, wq, bq, eps, noise) for L_ in (4, 8) for wq, bq in ((0, 0), (1, 1), (1, 0)) for eps in (0, 1) for noise in (0, 1)]


@pytest.mark.parametrize("L_,use_wq,use_bq,use_eps,use_noise", _FIN)
def test_vae_finish(L_, use_wq, use_bq, use_eps, use_noise):
    """quant_conv + reparameterisation + scaling + noise.  logvar takes values around -40, -30, 0, 20 and 25: both clamp limits are crossed."""
    lb, B, HW = lib(), 2, 37 * 29
    g = gen(100 * L_ + 8 * use_wq + 4 * use_bq + 2 * use_eps + use_noise)
    L2 = 2 * L_
    scaling, na, nb, in_scale = 0.18215, 0.8, 0.6, 0.75
    wq, sgn = _dominant(L2, g, L_) if use_wq else (None, torch.ones(L2))
    bq = torch.randn(L2, generator=g) * 0.05 if use_bq else None
    target = torch.empty(B * HW, L2)
    target[:, :L_] = _signed((B * HW, L_), 1.5, 2.5, g)
    lv = torch.tensor([-40.0, -30.0, 0.0, 20.0, 25.0])[torch.randint(0, 5, (B * HW, L_), generator=g)]
    target[:, L_:] = lv + (torch.rand(B * HW, L_, generator=g) - 0.5)
    h = target * sgn[None, :]                                 # through a +-1 diagonal the moments come out near `target`
    eps = _signed((B, L_, HW), 0.1, 0.3, g).half() if use_eps else None
    noise = _signed((B, L_, HW), 2.0, 3.0, g).half() if use_noise else None
    out = guard((B * L_ * HW + 100,), torch.float16)
    hd, wd, bd, ed, nd = [t.cuda() if t is not None else None for t in (h, wq, bq, eps, noise)]
    ok(lb.gdf_op_vae_finish(P(hd), B, HW, L_, P(wd), P(bd), P(ed), P(nd), scaling, na, nb, in_scale, P(out), stream()), lb)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(out.numel(), dtype=torch.bool)
    owned[:B * L_ * HW] = True
    assert_owned(got, owned)
    # float64 reference from the float32 values of the fp16 operands, with the magnitude sum of every output's terms
    f32 = lambda v: float(np.float32(v))
    h64 = h.double()
    if use_wq:
        m = h64 @ wq.double().t() + (bq.double() if use_bq else 0.0)
        mabs = h64.abs() @ wq.double().abs().t() + (bq.double().abs() if use_bq else 0.0)
    else:
        m, mabs = h64, h64.abs()
    nchw = lambda t: t.reshape(B, HW, L_).permute(0, 2, 1)
    z, zabs = nchw(m[:, :L_]), nchw(mabs[:, :L_])
    if use_eps:
        sd = torch.exp(0.5 * nchw(m[:, L_:]).clamp(-30.0, 20.0)) * eps.double()
        z, zabs = z + sd, zabs + sd.abs()
    ref, mag = f32(scaling) * z, f32(scaling) * zabs
    if use_noise:
        ref, mag = f32(na) * ref + f32(nb) * noise.double(), f32(na) * mag + f32(nb) * noise.double().abs()
    ref, mag = f32(in_scale) * ref, f32(in_scale) * mag
    assert bool((ref.abs() * 8.0 >= mag).all()) and float(ref.abs().max()) < 60000.0       # the premise of the bound (test inputs, not the kernel)
    u = ulps16(got[:B * L_ * HW].reshape(B, L_, HW), ref)
    print("vae_finish L=%d wq=%d bq=%d eps=%d noise=%d: max %d ulp, %.1f %% exact" % (L_, use_wq, use_bq, use_eps, use_noise, int(u.max()),
                                                                                      100.0 * float((u == 0).float().mean())))
    assert int(u.max()) <= 1


def test_vae_finish_refuses_more_than_8_latent_channels():
    lb = lib()
    h = torch.zeros(16, 18, device="cuda")
    out = guard((16 * 9 + 8,), torch.float16)
    refused(lb, lb.gdf_op_vae_finish(P(h), 1, 16, 9, None, None, None, None, 1.0, 1.0, 0.0, 1.0, P(out), stream()), "vae_finish")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


@pytest.mark.parametrize("L_,use_wq,use_bq,use_eps,B,HW", [(4, 0, 0, 0, 2, 37 * 29), (4, 1, 1, 1, 2, 37 * 29), (8, 1, 0, 0, 2, 37 * 29),
                                                           (8, 0, 0, 1, 2, 37 * 29), (8, 1, 1, 1, 2, 37 * 29),
                                                           (4, 1, 1, 1, 1, 1100 * 1000)])     # 1.1 M pixels > 4096 * 256: the stride loop
def test_vae_dec_prepare(L_, use_wq, use_bq, use_eps, B, HW):
    lb = lib()
    g = gen(10 * L_ + 4 * use_wq + 2 * use_bq + use_eps)
    ca, cb, inv_sf = 1.1, -0.7, 1.0 / 0.18215
    lat = _signed((B, L_, HW), 1.0, 2.0, g).half()
    eps = _signed((B, L_, HW), 0.1, 0.4, g).half() if use_eps else None
    wq = _dominant(L_, g)[0] if use_wq else None
    bq = torch.randn(L_, generator=g) * 0.05 if use_bq else None
    n = B * HW
    out = guard((n + 5, 8), torch.float16)
    ld, ed, wd, bd = [t.cuda() if t is not None else None for t in (lat, eps, wq, bq)]
    ok(lb.gdf_op_vae_dec_prepare(P(ld), P(ed), B, HW, L_, ca, cb, inv_sf, P(wd), P(bd), P(out), stream()), lb)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(n + 5, 8, dtype=torch.bool)
    owned[:n] = True
    assert_owned(got, owned)
    assert bool((bits(got[:n, L_:]) == 0).all())                                      # channels [L, 8) are +0
    f32 = lambda v: float(np.float32(v))
    z = f32(ca) * lat.double()
    zabs = z.abs()
    if use_eps:
        z, zabs = z + f32(cb) * eps.double(), zabs + (f32(cb) * eps.double()).abs()
    z, zabs = (z * f32(inv_sf)).permute(0, 2, 1).reshape(n, L_), (zabs * f32(inv_sf)).permute(0, 2, 1).reshape(n, L_)
    if use_wq:
        ref = z @ wq.double().t() + (bq.double() if use_bq else 0.0)
        mag = zabs @ wq.double().abs().t() + (bq.double().abs() if use_bq else 0.0)
    else:
        ref, mag = z, zabs
    assert bool((ref.abs() * 8.0 >= mag).all())
    u = ulps16(got[:n, :L_], ref)
    print("vae_dec_prepare L=%d wq=%d bq=%d eps=%d n=%d: max %d ulp" % (L_, use_wq, use_bq, use_eps, n, int(u.max())))
    assert int(u.max()) <= 1


# ------------------------------------------------------------------------------------------------------------------------------
# output-stage post-processing
# ------------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    """channels-last storage, like every hook"""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,W,S,Cc,f32,chlast,coff,extra", [
    (20, 136, 200, 16, 0, 1, 0, 0),        # non-square; the source row crosses the 128-pixel slab boundary while upsampling
    (192, 192, 160, 8, 0, 1, 0, 0),        # downsampling, two slabs
    (53, 53, 53, 8, 0, 1, 0, 0),
    (20, 136, 200, 70, 1, 0, 5, 9),        # fp32 NCHW-contiguous (sc = H W): one full and one partial 64-channel chunk, into channels [5, 75) of 79
    (12, 20, 30, 70, 0, 1, 5, 9)])
def test_resize_concat(H, W, S, Cc, f32, chlast, coff, extra):
    L, B = lib(), 2
    v = torch.randn(B, Cc, H, W, generator=gen(H + S))
    v = v if f32 else v.half()
    v = _cl(v) if chlast else v.contiguous()
    Ctot = Cc + extra
    out = guard((B, Ctot, S, S), torch.float16)
    vd = v.cuda()
    sb, sc, sy, sx = vd.stride()
    ok(L.gdf_op_resize_concat(P(vd), f32, sb, sc, sy, sx, B, Cc, H, W, P(out), Ctot, coff, S, stream()), L)
    torch.cuda.synchronize()
    want = guard((B, Ctot, S, S), torch.float16, "cpu")
    want[:, coff:coff + Cc] = F.interpolate(v.float(), (S, S)).half()
    assert_bits(out, want)


def test_resize_concat_refuses_channels_past_the_output():
    L = lib()
    v = torch.zeros(1, 8, 4, 4, dtype=torch.half, device="cuda")
    out = guard((1, 10, 4, 4), torch.float16)
    refused(L, L.gdf_op_resize_concat(P(v), 0, 128, 16, 4, 1, 1, 8, 4, 4, P(out), 10, 3, 4, stream()), "resize_concat")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


@pytest.mark.parametrize("heads", [1, 20])
@pytest.mark.parametrize("n", [1, 32])
def test_maps_mean(n, heads):
    """mean over heads, rounded to fp16 like the reference's `attention_probs.mean(1)`, then mean over the n maps.  Bound per element:
    2^-11 max_l(mean_l) + 2^-20 — one fp16 ulp of a per-layer head mean whose fp32 value rounds to the other fp16 neighbour than the exact
    mean does, plus the fp32 roundings of the sums."""
    L, B, Q, K = lib(), 2, 36, 77                             # Q K = 2772: not a multiple of 256
    g = gen(n * 100 + heads)
    maps = [(torch.rand(B, heads, Q, K, generator=g) * (2.0 / K)).half() for _ in range(n)]
    md = [m.cuda() for m in maps]
    out = guard((B * Q * K + 300,), torch.float32)
    ptrs = (vp * n)(*[m.data_ptr() for m in md])
    ok(L.gdf_op_maps_mean(ptrs, n, B, heads, Q, K, P(out), stream()), L)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(out.numel(), dtype=torch.bool)
    owned[:B * Q * K] = True
    assert_owned(got, owned)
    per = torch.stack([m.double().mean(1) for m in maps])                              # [n][B][Q][K] exact head means
    ref = per.to(torch.float16).double().mean(0).reshape(-1)
    bound = 2.0 ** -11 * per.max(0).values.reshape(-1) + 2.0 ** -20
    err = (got[:B * Q * K].double() - ref).abs()
    print("maps_mean n=%d heads=%d: max err / bound %.3f" % (n, heads, float((err / bound).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("n", [0, 33])
def test_maps_mean_refuses_bad_counts(n):
    L = lib()
    m = torch.zeros(1, 1, 4, 4, dtype=torch.half, device="cuda")
    out = guard((64,), torch.float32)
    ptrs = (vp * 33)(*[m.data_ptr()] * 33)
    refused(L, L.gdf_op_maps_mean(ptrs, n, 1, 1, 4, 4, P(out), stream()), "maps_mean")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())


def _pool_input(B, Cc, H, W, seed):
    """channels of one sign each, magnitudes in [0.5, 2): no window sum cancels, so the fp32 sum of <= 100 fp16 values is within
    100 * 2^-24 of the exact one, relatively, and the stored fp16 is the exact mean's rounding or a neighbour of it"""
    g = gen(seed)
    sgn = torch.randint(0, 2, (1, Cc, 1, 1), generator=g).float() * 2.0 - 1.0
    return _cl(((torch.rand(B, Cc, H, W, generator=g) * 1.5 + 0.5) * sgn).half())


def _avg_pool_op(L, x, r):
    B, Cc, H, W = x.shape
    OH, OW = H // r, W // r
    out = guard((B * OH * OW + 3, Cc), torch.float16)
    xd = x.cuda()
    assert xd.stride(1) == 1
    ok(L.gdf_op_avg_pool(P(xd), xd.stride(0), xd.stride(2), xd.stride(3), B, Cc, H, W, r, P(out), stream()), L)
    torch.cuda.synchronize()
    got = out.cpu()
    owned = torch.zeros(B * OH * OW + 3, Cc, dtype=torch.bool)
    owned[:B * OH * OW] = True
    assert_owned(got, owned)
    return got[:B * OH * OW].reshape(B, OH, OW, Cc).permute(0, 3, 1, 2)


POOL_DIV = [(32, 48, 2), (32, 48, 4), (32, 48, 8)]
POOL_REM = [(12, 8, 8), (33, 50, 2), (33, 50, 4), (65, 65, 8)]


@pytest.mark.parametrize("H,W,r", POOL_DIV + POOL_REM)
def test_avg_pool_matches_adaptive_avg_pool2d(H, W, r):
    """`feature_resize` is F.adaptive_avg_pool2d(feat, (H // r, W // r)): where r does not divide the size its windows are
    [floor(o H / OH), ceil((o + 1) H / OH)), longer than r and covering every row and column.  Within 1 fp16 ulp of the fp16-rounded
    float64 reference (see _pool_input)."""
    L = lib()
    x = _pool_input(2, 16, H, W, seed=H * W + r)
    ref = F.adaptive_avg_pool2d(x.double(), (H // r, W // r))
    u = ulps16(_avg_pool_op(L, x, r), ref)
    print("avg_pool %dx%d r=%d: max %d ulp, %.1f %% exact" % (H, W, r, int(u.max()), 100.0 * float((u == 0).float().mean())))
    assert int(u.max()) <= 1


@pytest.mark.parametrize("H,W,r", POOL_DIV)
def test_avg_pool_divisible_sizes_keep_their_bits(H, W, r):
    """where r divides H and W the window is the r x r block and the result is, bit for bit, fp16(fp32 sum in row-major window order *
    fp32(1 / r^2)): what the kernel computed before it learnt the adaptive windows"""
    L = lib()
    x = _pool_input(2, 16, H, W, seed=H * W + r)
    acc = torch.zeros(2, 16, H // r, W // r, dtype=torch.float32)
    for dy in range(r):
        for dx in range(r):
            acc = acc + x[:, :, dy::r, dx::r].float()         # IEEE fp32 additions in the kernel's order
    want = (acc * float(np.float32(1.0) / np.float32(r * r))).half()
    got = _avg_pool_op(L, x, r)
    assert torch.equal(bits(got.contiguous()), bits(want.contiguous()))


@pytest.mark.parametrize("H,W,r", POOL_REM)
def test_postproc_avg_pool_same_on_device_and_host(H, W, r):
    """components.postproc.avg_pool on a CUDA channels-last hook (the kernel) and on the same tensor on the CPU (ATen): both within 1 ulp of
    the reference and of each other — the same call no longer depends on where the tensor lives"""
    from components.postproc import avg_pool
    x = _pool_input(2, 16, H, W, seed=H * W + r)
    ref = F.adaptive_avg_pool2d(x.double(), (H // r, W // r))
    dev = avg_pool(x.cuda(), r)
    torch.cuda.synchronize()
    host = avg_pool(x, r)
    assert dev.is_cuda and dev.shape == host.shape == ref.shape and dev.dtype == host.dtype == torch.float16
    dev = dev.cpu()
    assert int(ulps16(dev, ref).max()) <= 1 and int(ulps16(host, ref).max()) <= 1
    assert int((ord16(dev) - ord16(host)).abs().max()) <= 1


def test_avg_pool_refuses_maps_smaller_than_the_window():
    L = lib()
    x = torch.zeros(1, 6, 12, 8, dtype=torch.half, device="cuda")                     # (B, H, W, C) storage: H = 6 < r = 8
    out = guard((64,), torch.float16)
    refused(L, L.gdf_op_avg_pool(P(x), 6 * 12 * 8, 12 * 8, 8, 1, 8, 6, 12, 8, P(out), stream()), "avg_pool")
    refused(L, L.gdf_op_avg_pool(P(x), 6 * 12 * 8, 12 * 8, 8, 1, 8, 12, 6, 8, P(out), stream()), "avg_pool")
    torch.cuda.synchronize()
    assert bool(is_guard(out.cpu()).all())
