"""Kernel-level parity of the MMDiT row kernels of csrc/dit.hip (-m gpu) in every form a plan uses: layernorm_mod_kernel<1, 2, 4, 6, 8>
(plain, split (hi, lo) pair, fp8 + row scale written in the same pass, fp16 source), quant_rows_fp8_kernel, qk_norm_rope_kernel<false, true>,
rope_table_kernel and softmax_rows_kernel, through gdf_op_layernorm_mod_ex and the existing gdf_op_* entry points.

Reference: float64 on the CPU, from the exact fp32 / 16-bit values handed to the kernel.  Every check is per element:
    |got - ref| <= u |ref| + slack          u = 2^-11 (fp16 storage) or 2^-8 (bf16 storage): one rounding to the output type
`slack` is what fp32 arithmetic costs and comes from no kernel: the same formula evaluated in plain torch float32 on the CPU, its largest
elementwise deviation from the float64 reference over the case, times SLACK_MARGIN = 8 (64 lanes sum in another order than torch does).
LN_CASES / QK_CASES record that deviation as it was measured when the case was written (`dev32`, slack = 8 dev32); a run computes it again
from the same function and prints both.

Buffers: whatever a kernel reads sits in a larger allocation whose padding columns and rows after the last hold POISON (1e4); whatever it
writes has SENT (0x5A bytes) in its padding columns and in rows >= R, compared bitwise afterwards.  R <= 7 rows everywhere.
tests/test_dit_rows_cpu.py checks without a GPU that LN_CASES reaches all five instantiations and the widths of the real models."""
import ctypes
import functools

import pytest
import torch

from oracle import flux_ref as FR
from ops_binding import P, lib, ok, rel, stream, vp

POISON = 1e4
SLACK_MARGIN = 8.0
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
EPS = 1e-6
R_LN = 7                                    # two workgroups of four waves: the last has three rows, its fourth wave leaves at `row >= R`

# sample of a row: row / rps below seg_rows (or seg_rows == 0), else (row - seg_rows) / rps2      (rps, seg_rows, rps2)
LN_MAPS = {"rps3": (3, 0, 1),               # samples 0 0 0 1 1 1 2
           "seg4": (2, 4, 2),               # text rows 0 0 1 1, image rows 0 0 1: the last sample is a single row
           "seg4x3": (2, 4, 3)}             # rps2 != rps (image rows 0 0 0): the second segment must divide by rps2
# C: (MAXC it takes, fp32-vs-fp64 deviation of the formula for the maps rps3 / seg4 / seg4x3 and, last, the fp16-source case) -- measured on the
# CPU by ln_problem(); the slack of a case is 8 x its entry.  The row of mean 1000 sets it: its fp32 mean is rounded to a grid of 6e-5, which
# (1 + scale) multiplies; where the mean happens to round well (C = 8 / rps3) the figure is that of the other rows, ~1e-7.
LN_WIDTHS = {
    8: (1, dict(rps3=1.3e-07, seg4=5.2e-05)),
    512: (1, dict(rps3=2.9e-05, seg4=1.6e-04)),
    520: (2, dict(rps3=1.2e-04, seg4=9.5e-05, x16=1.9e-05)),
    1024: (2, dict(rps3=3.0e-05, seg4=6.2e-06)),
    1152: (4, dict(rps3=4.6e-04, seg4=4.5e-05, seg4x3=3.5e-04)),
    2048: (4, dict(rps3=1.4e-04, seg4=2.1e-04)),
    2056: (6, dict(rps3=5.3e-05, seg4=9.5e-05)),
    3072: (6, dict(rps3=2.7e-04, seg4=1.0e-05, seg4x3=1.4e-04, x16=1.0e-04)),
    3080: (8, dict(rps3=3.3e-04, seg4=8.4e-05)),
    4096: (8, dict(rps3=1.8e-05, seg4=7.3e-06)),
}


def _ln_cases():
    out = []
    for C, (maxc, d32) in LN_WIDTHS.items():
        forms = ["f16", "bf16", "bf16-pair", "bf16-q8"] + (["f16-pair"] if C in (1152, 3072) else []) + (["x16-f16"] if C in (520, 3072) else [])
        for form in forms:
            for m in ("rps3", "seg4"):
                d = d32["x16"] if form == "x16-f16" else d32[m]
                out.append(dict(id="C%d-%s-%s" % (C, form, m), C=C, maxc=maxc, form=form, map=m, dev32=d, slack=SLACK_MARGIN * d))
        if "seg4x3" in d32:
            out.append(dict(id="C%d-bf16-seg4x3" % C, C=C, maxc=maxc, form="bf16", map="seg4x3", dev32=d32["seg4x3"], slack=SLACK_MARGIN * d32["seg4x3"]))
    return out


LN_CASES = _ln_cases()


def dev(t):
    return t.cuda()


def sent(shape, dtype):
    """a device buffer of 0x5A bytes"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0x5A)
    return t


def all_sent(t):
    return bool((t.contiguous().view(torch.uint8) == 0x5A).all())


def check_elementwise(got, ref, u, slack, what, extra=0.0):
    """|got - ref| <= u |ref| + slack + extra for every element (float64 on the CPU)"""
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    bound = u * ref.abs() + slack + extra
    over = err - bound
    i = int(over.argmax())
    assert bool((err <= bound).all()), "%s: element %s got %r ref %r err %.3e bound %.3e" % (
        what, tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)), float(got.flatten()[i]), float(ref.flatten()[i]),
        float(err.flatten()[i]), float(bound.flatten()[i]))


def check_row_scales(scale, amax, what):
    """a power of two with 224 <= amax / scale <= 448 (1 for a zero row); at amax = 448 2^k both neighbours pass"""
    scale, amax = scale.double().cpu(), amax.double()
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all()), (what, scale)
    z = amax == 0
    assert bool((scale[z] == 1).all()), (what, scale)
    ratio = amax[~z] / scale[~z]
    assert bool(((ratio >= 224) & (ratio <= 448)).all()), (what, ratio)


def e4m3_half_ulp(a):
    """half the spacing of OCP e4m3 around |a| (float64): 2^(e - 4) in the binade [2^e, 2^(e + 1)), the subnormal step 2^-9 below 2^-6"""
    a = a.abs()
    _, ex = torch.frexp(a)
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, -6)).clamp(min=-6, max=8)
    return torch.ldexp(torch.ones_like(a), e - 4)


# ------------------------------------------------------------------------------------------------------------------ layernorm_mod
def ln_sample(m, R):
    rps, seg, rps2 = LN_MAPS[m]
    return torch.tensor([(r - seg) // rps2 if seg > 0 and r >= seg else r // rps for r in range(R)])


@functools.lru_cache(maxsize=None)
def ln_problem(C, m, x16):
    """inputs (CPU), float64 reference of the modulated rows and the measured fp32 deviation of one (C, sample map, source type)"""
    R = R_LN
    g = torch.Generator().manual_seed(1000 * C + 10 * list(LN_MAPS).index(m) + (7 if x16 else 0))
    x = torch.randn(R, C, generator=g)
    x[1] = 1000.0 + torch.randn(C, generator=g)             # a one-pass variance E[x^2] - mean^2 is off by ~6e-2 here
    x[2] = 2.5                                               # variance 0 (every partial sum of 2.5 is exact in fp32): y == shift
    x[3, C - 1] = 1e4                                        # one outlier, in the last column (the last active lane's last element)
    x[6] = x[6] * 3 + 0.5
    if x16:
        x = x.half().float()
    smp = ln_sample(m, R)
    nsmp = int(smp.max()) + 1
    ldm = 2 * C + 16                                         # [4 | shift C | 4 | scale C | 4 ...]: both pointers at column offsets of one matrix
    mod = torch.full((nsmp + 1, ldm), POISON)
    mod[:nsmp, 4:4 + C] = torch.randn(nsmp, C, generator=g)
    mod[:nsmp, C + 8:2 * C + 8] = torch.randn(nsmp, C, generator=g)
    sh, sc = mod[smp, 4:4 + C], mod[smp, C + 8:2 * C + 8]
    xd = x.double()
    d = xd - xd.mean(-1, keepdim=True)
    ref = d / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS) * (1 + sc.double()) + sh.double()
    d32 = x - x.mean(-1, keepdim=True)                       # the same formula in fp32
    t32 = d32 * torch.rsqrt((d32 * d32).mean(-1, keepdim=True) + torch.tensor(EPS)) * (1.0 + sc) + sh
    dev32 = float((t32.double() - ref).abs().max())
    return dict(x=x, mod=mod, ldm=ldm, ref=ref, dev32=dev32, slack=SLACK_MARGIN * dev32)


def ln_launch(L, prob, C, m, dt, x16=False, pair=False, q8=False, over=None):
    """one gdf_op_layernorm_mod_ex launch on fresh device buffers; returns rc and the raw output buffers"""
    R, ld = R_LN, C + 8
    xb = torch.full((R + 1, ld), POISON)
    xb[:R, :C] = prob["x"]
    xb = dev(xb.half() if x16 else xb)
    mod = dev(prob["mod"])
    ldy, y_lo = (2 * C + 8, C) if pair else (C + 8, 0)
    y = sent((R + 2, ldy), torch.int16)
    q = sent((R + 2, C + 8), torch.uint8) if q8 else None
    qs = sent((R + 2,), torch.float32) if q8 else None
    rps, seg, rps2 = LN_MAPS[m]
    a = dict(x16=P(xb) if x16 else vp(0), x32=vp(0) if x16 else P(xb), ld=ld, C=C, scale=vp(mod.data_ptr() + 4 * (C + 8)), shift=vp(mod.data_ptr() + 4 * 4),
             ldy=ldy, y_lo=y_lo, q8=P(q), ldq8=C + 8, q8_scale=P(qs))
    a.update(over or {})
    rc = L.gdf_op_layernorm_mod_ex(a["x16"], a["x32"], a["ld"], R, a["C"], EPS, a["scale"], a["shift"], prob["ldm"], rps, seg, rps2, P(y),
                                   int(dt == torch.bfloat16), a["ldy"], a["y_lo"], a["q8"], a["ldq8"], a["q8_scale"], stream())
    torch.cuda.synchronize()
    return rc, y, q, qs


@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_CASES, ids=[c["id"] for c in LN_CASES])
def test_layernorm_mod_forms(c):
    L = lib()
    C, m, form, R = c["C"], c["map"], c["form"], R_LN
    assert L.gdf_op_layernorm_mod_path(C) == c["maxc"]
    x16 = form == "x16-f16"
    dt = torch.bfloat16 if form.startswith("bf16") else torch.float16
    u = U[dt]
    prob = ln_problem(C, m, x16)
    ref, slack = prob["ref"], prob["slack"]
    print("%s: fp32-vs-fp64 deviation %.2e (recorded %.2e), slack %.2e" % (c["id"], prob["dev32"], c["dev32"], slack))
    rc, y, _, _ = ln_launch(L, prob, C, m, dt, x16=x16)
    ok(rc, L)
    plain = y[:R, :C].view(dt).cpu()
    check_elementwise(plain, ref, u, slack, c["id"])
    assert all_sent(y[:R, C:]) and all_sent(y[R:]), "plain form wrote outside its rows"
    if form.endswith("pair"):
        rc, y2, _, _ = ln_launch(L, prob, C, m, dt, pair=True)
        ok(rc, L)
        hi, lo = y2[:R, :C].view(dt).cpu(), y2[:R, C:2 * C].view(dt).cpu()
        assert torch.equal(y2[:R, :C].cpu(), y[:R, :C].cpu()), "hi of the pair differs from the plain output"
        check_elementwise(hi.double() + lo.double(), ref, 2 * u * u, slack, c["id"] + " hi+lo", extra=2.0 ** -25 if dt == torch.float16 else 0.0)
        assert all_sent(y2[:R, 2 * C:]) and all_sent(y2[R:]), "pair form wrote outside its rows"
    if form.endswith("q8"):
        rc, y2, q, qs = ln_launch(L, prob, C, m, dt, q8=True)
        ok(rc, L)
        assert torch.equal(y2.cpu(), y.cpu()), "16-bit output changes when the fp8 row is written too"
        s = qs[:R].cpu().double()
        check_row_scales(s, ref.abs().amax(-1), c["id"])
        deq = q[:R, :C].view(torch.float8_e4m3fn).cpu().float().double() * s[:, None]
        err, bound = (deq - ref).abs(), e4m3_half_ulp(ref / s[:, None]) * s[:, None] + slack
        assert bool((err <= bound).all()), "%s fp8 row: worst excess %.3e (the bytes are not the fp32 values rounded once)" % (c["id"], float((err - bound).max()))
        assert all_sent(q[:R, C:]) and all_sent(q[R:]) and all_sent(qs[R:]), "fp8 form wrote outside its rows"


# ------------------------------------------------------------------------------------------------------------------ quant_rows_fp8
def next_up(v, dt):
    return (torch.tensor(v, dtype=dt).view(torch.int16) + 1).view(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 2048, 2056, 3072])       # 2056, 3072: a second trip of the 2048-column loop with 1 and 128 of 256 lanes
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_quant_rows_fp8(dt, K):
    L = lib()
    R, ld, ldq = 6, K + 8, K + 8
    g = torch.Generator().manual_seed(K)
    x = torch.randn(R, K, generator=g).to(dt)
    x[1] = 0                                                 # scale exactly 1, every byte 0
    body = (torch.randn(2, K, generator=g).clamp(-3, 3) * 10).to(dt)
    x[2], x[3] = body[0], body[1]
    x[2, K - 3] = 448 * 2.0 ** -3                            # amax / 448 is a power of two: `amax * (1 / 448.f)` is a rounded product
    x[3, K - 3] = next_up(448 * 2.0 ** -3, dt)               # one 16-bit step above it: only the larger scale keeps the row below 448
    x[4, K - 1] = -1000.0                                    # the row maximum is the last element read, and negative
    if dt == torch.float16:
        x[5] = (torch.randint(-1023, 1024, (K,), generator=g).double() * 2.0 ** -24).to(dt)      # fp16 subnormals
        x[5, 0] = 1023 * 2.0 ** -24
    else:
        x[5] = (torch.randn(K, generator=g) * 100).to(dt)
    xb = torch.full((R + 1, ld), POISON).to(dt)
    xb[:R, :K] = x
    xb = dev(xb)
    q, sc = sent((R + 2, ldq), torch.uint8), sent((R + 2,), torch.float32)
    ok(L.gdf_op_quant_rows_fp8(P(xb), ld, R, K, int(dt == torch.bfloat16), P(q), ldq, P(sc), stream()), L)
    torch.cuda.synchronize()
    s = sc[:R].cpu()
    check_row_scales(s, x.double().abs().amax(-1), "quant_rows_fp8")
    assert float(s[1]) == 1.0 and bool((q[1, :K] == 0).all())
    got = q[:R, :K].cpu()
    want = (x.float() / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)       # a power-of-two division is exact: ties round alike
    same = (got == want) | (((got & 0x7F) == 0) & ((want & 0x7F) == 0))
    assert bool(same.all()), "%d bytes differ from the CPU cast, first at %s" % (int((~same).sum()), (~same).nonzero()[0].tolist())
    assert all_sent(q[:R, K:]) and all_sent(q[R:]) and all_sent(sc[R:])


# ------------------------------------------------------------------------------------------------------------------ qk_norm_rope
# fp32-vs-fp64 deviation of RMSNorm + RoPE over a case (measured on the CPU by qk_problem) -> slack = 8 x
QK_DEV32 = {("f16", 1, "wrap"): 4.1e-07, ("f16", 1, "flat"): 4.8e-07, ("f16", 3, "wrap"): 5.1e-07, ("f16", 3, "flat"): 4.6e-07,
            ("bf16", 1, "wrap"): 3.4e-07, ("bf16", 1, "flat"): 6.6e-07, ("bf16", 3, "wrap"): 4.9e-07, ("bf16", 3, "flat"): 5.5e-07}
QK_POS = {"wrap": (5, 4), "flat": (0, 7)}                   # (pos0, rps): positions 5 6 7 8 5 6 7 wrap across samples / 0..6
QK_CASES = [dict(id="%s-h%d-%s-%s" % (dn, h, lay, pos), dt=dt, heads=h, layout=lay, pos=pos, dev32=QK_DEV32[(dn, h, pos)], slack=SLACK_MARGIN * QK_DEV32[(dn, h, pos)])
            for dn, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)) for h in (1, 3) for lay in ("qkv", "vkq") for pos in ("wrap", "flat")]


@functools.lru_cache(maxsize=None)
def qk_problem(dt, heads, pos):
    """16-bit q / k heads, gains, the cos / sin table, the float64 reference of both and the fp32 deviation (the same for both layouts)"""
    R, D = 7, 128
    pos0, rps = QK_POS[pos]
    g = torch.Generator().manual_seed(17 * heads + pos0)
    qk = torch.randn(2, R, heads, D, generator=g)
    qk[:, 2] *= 30.0                                         # rows of another magnitude: the norm is per (row, head)
    qk[:, 4, heads - 1] = 0                                  # one (row, head) of zeros -> exactly 0
    qk = qk.to(dt)
    w = 1 + 0.1 * torch.randn(2, D, generator=g)
    npos = pos0 + rps + 2
    ids = torch.stack([torch.arange(npos) * 0.5, torch.arange(npos) * 9.0, 127.0 - torch.arange(npos)], 1)
    cos, sin = FR.rope_freqs(ids, (16, 56, 56))
    p = pos0 + torch.arange(R) % rps

    def formula(v, w, c, s):                                 # v (R, heads, D)
        v = v * torch.rsqrt((v * v).mean(-1, keepdim=True) + EPS) * w
        rot = torch.stack([-v[..., 1::2], v[..., 0::2]], -1).flatten(-2)
        return v * c[p][:, None] + rot * s[p][:, None]

    ref = torch.stack([formula(qk[i].double(), w[i].double(), cos.double(), sin.double()) for i in range(2)])
    f32 = torch.stack([formula(qk[i].float(), w[i], cos, sin) for i in range(2)])
    dev32 = float((f32.double() - ref).abs().max())
    tab = torch.full((2, npos, D), POISON)                   # table rows no row of this launch maps to: never read
    tab[0, pos0:pos0 + rps], tab[1, pos0:pos0 + rps] = cos[pos0:pos0 + rps], sin[pos0:pos0 + rps]
    return dict(qk=qk, w=w, tab=tab, ref=ref, dev32=dev32, slack=SLACK_MARGIN * dev32)


@pytest.mark.gpu
@pytest.mark.parametrize("c", QK_CASES, ids=[c["id"] for c in QK_CASES])
def test_qk_norm_rope_layouts(c):
    L = lib()
    dt, heads, R, D = c["dt"], c["heads"], 7, 128
    C = heads * D
    prob = qk_problem(dt, heads, c["pos"])
    print("%s: fp32-vs-fp64 deviation %.2e (recorded %.2e), slack %.2e" % (c["id"], prob["dev32"], c["dev32"], prob["slack"]))
    if c["layout"] == "qkv":                                 # [q | k | v | 8]
        ld, q_col, k_col = 3 * C + 8, 0, C
    else:                                                    # [v | 8 | k | 8 | q]
        ld, q_col, k_col = 3 * C + 16, 2 * C + 16, C + 8
    g = torch.Generator().manual_seed(3)
    xb = torch.full((R + 1, ld), POISON)
    v_col = 2 * C if c["layout"] == "qkv" else 0
    xb[:R, v_col:v_col + C] = torch.randn(R, C, generator=g)
    xb = xb.to(dt)
    xb[:R, q_col:q_col + C] = prob["qk"][0].reshape(R, C)
    xb[:R, k_col:k_col + C] = prob["qk"][1].reshape(R, C)
    before = xb.clone()
    xb, w, tab = dev(xb), dev(prob["w"]), dev(prob["tab"])
    pos0, rps = QK_POS[c["pos"]]
    ok(L.gdf_op_set_e16(2 if dt == torch.bfloat16 else 0), L)
    try:
        rc = L.gdf_op_qk_norm_rope(P(xb), ld, R, heads, q_col, k_col, P(w[0]), P(w[1]), EPS, P(tab[0]), P(tab[1]), pos0, rps, stream())
        torch.cuda.synchronize()
    finally:
        L.gdf_op_set_e16(0)
    ok(rc, L)
    got = xb.cpu()
    for i, col in ((0, q_col), (1, k_col)):
        out = got[:R, col:col + C].reshape(R, heads, D)
        check_elementwise(out, prob["ref"][i], U[dt], prob["slack"], "%s %s" % (c["id"], "qk"[i]))
        assert bool((out[4, heads - 1] == 0).all()), "a zero (row, head) must stay zero"
    keep = torch.ones(R + 1, ld, dtype=torch.bool)
    keep[:R, q_col:q_col + C] = False
    keep[:R, k_col:k_col + C] = False
    assert torch.equal(got.view(torch.int16)[keep], before.view(torch.int16)[keep]), "columns outside the q / k heads changed"


# ------------------------------------------------------------------------------------------------------------------ rope_table
@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 9])                       # 320 and 576 threads: one workgroup and a partial one, two and a partial third
def test_rope_table_rows(S):
    L = lib()
    axes, row0 = (16, 56, 56), 3
    r = torch.arange(S, dtype=torch.float32)
    ids = torch.stack([r * 0.75 + 0.25, 127.0 - 13.0 * r, (r * 31.0 + 3.0) % 128.0], 1).contiguous()
    ids[S - 1, 2] = 127.0
    cos, sin = sent((row0 + S + 2, 128), torch.float32), sent((row0 + S + 2, 128), torch.float32)
    ok(L.gdf_op_rope_table(P(dev(ids)), S, axes[0], axes[1], axes[2], P(cos), P(sin), row0, stream()), L)
    torch.cuda.synchronize()
    ang = torch.cat([torch.outer(ids[:, i].double(), 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float64) / d))).repeat_interleave(2, 1)
                     for i, d in enumerate(axes)], 1)
    for got, want in ((cos, ang.cos()), (sin, ang.sin())):
        assert float((got[row0:row0 + S].cpu().double() - want).abs().max()) <= 1e-6
        assert all_sent(got[:row0]) and all_sent(got[row0 + S:])


# ------------------------------------------------------------------------------------------------------------------ softmax_rows
@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 2056, 16384])             # one lane; 257 vectors: one lane takes a second chunk; every register chunk full
def test_softmax_rows_padded(n):
    L = lib()
    R, ld, scale = 5, n + 8, 0.0442
    g = torch.Generator().manual_seed(n)
    x = torch.randn(R, n, generator=g) * 20
    x[1] = 3.25                                              # all equal: 1 / n
    x[2, torch.randperm(n, generator=g)[:n // 2]] = -65504.0 # masked entries: exactly 0
    x[3] = torch.randn(n, generator=g)
    x[3, n - 1] = 400.0                                      # one dominant entry, in the last column
    x = x.half()
    xb = torch.full((R + 1, ld), POISON).half()
    xb[:R, :n] = x
    before = xb.clone()
    xb = dev(xb)
    ok(L.gdf_op_softmax_rows(P(xb), ld, R, n, ctypes.c_float(scale), stream()), L)
    torch.cuda.synchronize()
    got = xb.cpu()
    y = got[:R, :n]
    p = torch.softmax(x.double() * float(torch.tensor(scale)), -1)
    check_elementwise(y, p, U[torch.float16], 2.0 ** -24, "softmax n=%d" % n)
    assert bool((y[2][x[2] == -65504.0] == 0).all())
    assert rel(y, p) < 2e-3 and torch.allclose(y.float().sum(-1), torch.ones(R), atol=5e-3)
    keep = torch.ones(R + 1, ld, dtype=torch.bool)
    keep[:R, :n] = False
    assert torch.equal(got.view(torch.int16)[keep], before.view(torch.int16)[keep]), "padding changed"


# ------------------------------------------------------------------------------------------------------------------ rejected arguments
@pytest.mark.gpu
def test_rejected_arguments_launch_nothing():
    """host checks that return before any device call: an error code, and every output stays at the sentinel"""
    L = lib()
    C, m = 520, "rps3"
    prob = ln_problem(C, m, False)
    one = sent((8,), torch.float32)
    for what, kw, over in (("C above the largest instantiation", {}, dict(C=4104)), ("C % 8", {}, dict(C=12)), ("ld % 4 of an fp32 source", {}, dict(ld=C + 2)),
                           ("y_lo % 8", dict(pair=True), dict(y_lo=4)), ("q8 without q8_scale", dict(q8=True), dict(q8_scale=vp(0))),
                           ("both sources", {}, dict(x16=P(one)))):
        rc, y, q, qs = ln_launch(L, prob, C, m, torch.float16, over=over, **kw)
        assert rc != 0 and b"layernorm_mod_ex" in L.gdf_last_error(), what
        assert all_sent(y) and (q is None or (all_sent(q) and all_sent(qs))), what
    x = dev(torch.zeros(8, 16400).half())
    q, sc = sent((8, 16400), torch.uint8), sent((8,), torch.float32)
    assert L.gdf_op_quant_rows_fp8(P(x), 24, 4, 12, 0, P(q), 24, P(sc), stream()) != 0 and b"quant_rows_fp8" in L.gdf_last_error()
    torch.cuda.synchronize()
    assert all_sent(q) and all_sent(sc)
    y = sent((8, 16400), torch.int16)
    w, tab = dev(torch.ones(128)), dev(torch.ones(8, 128))
    assert L.gdf_op_qk_norm_rope(P(y), 512, 4, 1, 4, 256, P(w), P(w), EPS, P(tab), P(tab), 0, 4, stream()) != 0 and b"qk_norm_rope" in L.gdf_last_error()
    assert L.gdf_op_softmax_rows(P(y), 16400, 4, 16392, ctypes.c_float(1.0), stream()) != 0 and b"softmax_rows" in L.gdf_last_error()
    torch.cuda.synchronize()
    assert all_sent(y)
