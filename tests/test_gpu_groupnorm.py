"""Kernel-level parity of every producer of the GroupNorm affine table ab[b][c] = (rstd gamma, beta - mean rstd gamma) (-m gpu):
  fused   gn_fused_kernel (one launch, <= 32 x 32 pixels; the table stays in LDS),
  stats   gn_partial_kernel + gn_finalize_kernel (gdf_op_gn_stats),
  conv    the six gemm_gn_kernel instantiations whose epilogue writes per-slab channel sums, then gdf_op_gn_finalize (+ gn_fold_kernel),
and the LayerNorm template widths.  CASES is the map from kernel form to the test that runs it; tests/test_groupnorm_paths_cpu.py
asserts without a GPU that every form the shipped models reach has a row, and runs the emulation check below on every row.

References are fp64 on the CPU from the same fp16-rounded inputs.  Every output buffer is over-allocated and filled with a sentinel
that is compared bit for bit afterwards.  Bounds:
  benign inputs (|mean| / std <= 1)   |a - a_ref| <= 2e-6 |a_ref|,  |b - b_ref| <= 2e-6 (|beta| + |mean a|)            (TOL_AB)
  mean / std = 32 over the group      relative error of rstd (= of a / gamma) <= 3.3e-4: a third of the fp16 output bound  (TOL_RSTD32)
  mean / std = 128                    a characterisation: finite, output relative L2 < 1e-2 (the var < 0 -> 0 clamp is off by 1/sqrt(eps))
  per-slab channel sums of a conv     relative L2 over channels, worst slab, 2e-4 (TOL32: they are the fp32 accumulators the fp32 store gets)
  outputs y                           relative L2 1e-3 (TOL16)
emulate_sums() is a NumPy model of the kernels' summation order (fp32 running sums per thread, fp32 or double across threads as the
kernel has it, double across slabs); a case asserts that the emulation stays within a third of each bound it uses before it looks at
the GPU: every bound is reachable by a correct kernel, and the inputs, not the bounds, are what changes if that fails.
The fused kernel has no table: it is recovered per (sample, channel) by least squares from a silu = 0 run with fp32 input and a split
(hi, lo) output (22 mantissa bits; the fit over HW >= 64 points adds < 1e-7).
Every case prints its figures as a GN_CASE line (-s); the emulated envelope per path is in DESIGN.md 3.3.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ops_binding import P, lib, stream

TOL16, TOL32 = 1e-3, 2e-4
TOL_AB, TOL_RSTD32, TOL_Y128 = 2e-6, 3.3e-4, 1e-2
SENT16 = 0x5A5A                   # fp16 205.25
SENT32 = 0x5A5A5A5A               # fp32 1.5e16
RATIOS = (0, 32, 128)             # 0: benign (mean / std about 0.25)


def seed_of(s):
    return zlib.crc32(s.encode())


# ------------------------------------------------------------------------------------------------------------------------------
# CASES
# ------------------------------------------------------------------------------------------------------------------------------
def fused(C, HW, B=2, G=32, eps=1e-5, **kw):
    return dict(id="fused-c%d-hw%d%s" % (C, HW, "-g%d" % G if G != 32 else ""), path="fused", B=B, HW=HW, C=C, G=G, eps=eps, **kw)


def stats(id, B, HW, C, G=32, eps=1e-5, **kw):
    return dict(id="stats-" + id, path="stats", B=B, HW=HW, C=C, G=G, eps=eps, **kw)


def conv(id, kernel, variant, B, H, W, Cout, G=32, **kw):
    return dict(id="conv-" + id, path="conv", kernel=kernel, variant=variant, B=B, H=H, W=W, Cin=64, C=Cout, G=G, eps=1e-5, **kw)


def GK(mode, bm, bn, st):
    return "gemm_gn_kernel<%d, %d, %d, %d>" % (mode, bm, bn, st)


K128, K160, K256, K826, K932, KIN = GK(1, 128, 128, 2), GK(1, 128, 160, 2), GK(1, 256, 128, 3), GK(1, 256, 256, 8), GK(1, 256, 320, 9), GK(2, 128, 128, 2)

CASES = (
    # ---- fused: 2 / 4 / 10 / 12 (SC = 96: 252 active threads) / 16 / 30 / 80 channels per group, HW = 64, 100 (ragged rows), 1024 ----
    [fused(C, HW) for C in (64, 128, 320, 384, 512, 960, 2560) for HW in (64, 100, 1024)]
    + [fused(C, 100) for C in (640, 1280, 1920)]                             # 20 / 40 / 60 channels per group (UNet widths)
    + [fused(64, 100, G=8), fused(320, 64, eps=1e-6, id_suffix="eps"), fused(320, 100, ld_pad=64, id_suffix="ld"),
       fused(128, 100, pair_in=True, id_suffix="pairin")]
    # ---- statistics pass.  row groups = 256 / (C / 8); `unrolled`: the slab is long enough for the four-rows-in-flight loop ----
    + [stats("c320-hw4096", 1, 4096, 320, slab=16),                          # slab 16, six row groups, short loop only
       stats("c320-hw1100-ragged", 1, 1100, 320, slab=16),                   # ragged last slab (12 rows)
       stats("c64-slab64", 2, 65536, 64, slab=64),                           # B HW = 131072: slab 64, 32 row groups
       stats("c320-slab32-unrolled", 1, 40000, 320, slab=32),                # 32 rows over 6 row groups: four rows in flight
       stats("c128-slab64-unrolled", 1, 67600, 128, slab=64),                # 16 row groups
       stats("c256-slab32-unrolled", 1, 34900, 256, slab=32),                # 8 row groups
       stats("c128", 1, 1100, 128, slab=16),                                 # 16 row groups, short loop only
       stats("c256", 1, 1100, 256, slab=16),                                 # 8
       stats("c512", 1, 1100, 512, slab=16),                                 # 4 row groups
       stats("c640", 1, 1100, 640, slab=16),                                 # 3
       stats("c960", 1, 1100, 960, slab=16),                                 # 2
       stats("c1280", 1, 1100, 1280, slab=16),                               # 1 (160 of 256 threads)
       stats("c1920", 2, 1100, 1920, slab=16),                               # 1 (240 of 256 threads)
       stats("c2560-colloop", 2, 1100, 2560, slab=16),                       # C / 8 > 256: the column loop
       stats("c320-ld", 2, 1100, 320, slab=16, ld_pad=64),
       stats("c320-f32", 2, 1100, 320, slab=16, f32=True),
       stats("c320-pairin", 2, 1100, 320, slab=16, pair_in=True),
       stats("c320-pairout", 2, 1100, 320, slab=16, pair_out=True),
       stats("c64-g8", 2, 1100, 64, G=8, slab=16),
       stats("c320-eps1e-6", 2, 1100, 320, eps=1e-6, slab=16)]
    # ---- conv epilogue: bias + temb row vector + fp32 residual + aux16 on every kernel ----
    + [conv("128-m64", K128, 128, 1, 8, 8, 64),                              # half a tile: the second wave row owns no slab
       conv("128-m192-n72", K128, 128, 1, 16, 12, 72, G=8),                  # ragged column tile, three slabs in one sample
       conv("128-stride2", K128, 128, 3, 16, 16, 64, stride=2),
       conv("160-m192-n320", K160, 160, 3, 8, 8, 320),
       conv("160-ups", K160, 160, 3, 4, 4, 320, ups=1),
       conv("256-m320-n128", K256, 256, 5, 8, 8, 128),                       # 5 slabs in 1.25 tiles
       conv("826-m320-n256", K826, 826, 1, 20, 16, 256),
       conv("826-persistent", K826, 826, 65, 16, 16, 1024, ratios=(0,)),     # 260 tiles > 256 CUs: a workgroup's sums restart
       conv("932-m384-n320", K932, 932, 3, 16, 8, 320),                      # 128-row slabs
       conv("932-scale", K932, 932, 3, 16, 8, 320, scale=2.0 ** -6, ratios=(0,)),
       conv("932-persistent", K932, 932, 33, 16, 16, 2560, ratios=(0,)),     # 264 tiles
       conv("in-m192", KIN, 0, 3, 8, 8, 64, G=8, conv_in=True)]               # (8 channels per group: 512 values settle the group's std)
)
for _c in CASES:
    if "id_suffix" in _c:
        _c["id"] += "-" + _c.pop("id_suffix")

# fold: synthetic per-slab sums, B = 2
FOLD_CASES = [(300, 64), (300, 128), (300, 256), (300, 512), (300, 320), (300, 640), (256, 64), (257, 64), (257, 256)]
LN_CASES = [(5, 512), (7, 520), (5, 1024), (6, 1032), (5, 2048)]          # C / 8 = 64 / 65 / 128 / 129 / 256; R % 4 != 0


# ------------------------------------------------------------------------------------------------------------------------------
# host-only queries
# ------------------------------------------------------------------------------------------------------------------------------
def gn_path(L, B, HW, C, G):
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.gdf_op_gn_path(B, HW, C, G, a, b, c) == 0
    return a.value, b.value, c.value


def conv_info(L, B, H, W, Cin, Cout, stride, ups, variant):
    s = ctypes.c_int()
    n = L.gdf_op_conv3x3_gn_info(B, H, W, Cin, Cout, stride, ups, variant << 8, s)
    return (n.decode() if n is not None else None), s.value


def fold_shape(nslab, C):
    """(threads per slab row, row groups) of gn_fold_kernel, or None where launch_gn_finalize gathers unfolded"""
    C2 = 2 * C
    if nslab <= 256 or not (C2 % 1024 == 0 if C2 >= 1024 else 256 % (C2 // 4) == 0):
        return None
    tpr = min(256, C2 // 4)
    return tpr, 256 // tpr


def partial_form(C, slab):
    """row-group form of gn_partial_kernel: (row groups, column loop, four-rows-in-flight loop runs)"""
    CH = C // 8
    rg = 256 // min(CH, 256)
    return rg, CH > 256, slab > 3 * rg


def case_forms(c, L):
    """the kernel forms a case runs (what tests/test_groupnorm_paths_cpu.py compares with the forms the models reach)"""
    cpg = c["C"] // c["G"]
    if c["path"] == "fused":
        return {("fused", cpg)}
    if c["path"] == "stats":
        _, slab, _ = gn_path(L, c["B"], c["HW"], c["C"], c["G"])
        return {("partial",) + partial_form(c["C"], slab), ("finalize", cpg)}
    return {("epilogue", c["kernel"]), ("finalize", cpg), ("fold", None)}


# ------------------------------------------------------------------------------------------------------------------------------
# data, fp64 reference, emulation
# ------------------------------------------------------------------------------------------------------------------------------
def affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(C, generator=g)).float(), (0.1 * torch.randn(C, generator=g)).float()


def gn_input(c, ratio):
    """fp16-rounded x (B, HW, C) as fp64 with mean / std = ratio over every group (0: about 0.25).  std 2 keeps the noise 16 (ratio 32)
    or 8 (ratio 128) fp16 ulps wide."""
    g = torch.Generator().manual_seed(seed_of(c["id"]) + ratio)
    x = 2.0 * torch.randn(c["B"], c["HW"], c["C"], generator=g) + (0.5 if ratio == 0 else 2.0 * ratio)
    return x.half()


def split16(x32):
    hi = x32.half()
    return hi, (x32 - hi.float()).half()


def group_stats(x64, G):
    """x64 (B, HW, C) -> mean, var (B, G) fp64 (biased variance)"""
    B, HW, C = x64.shape
    xg = x64.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    return xg.mean(-1), xg.var(-1, unbiased=False)


def ab_from(mean, var, eps, gamma, beta, C):
    """fp64 table from group statistics -> a, b (B, C), rstd, mean per channel"""
    cpg = C // mean.shape[1]
    rstd = (var + eps).rsqrt().repeat_interleave(cpg, 1)
    m = mean.repeat_interleave(cpg, 1)
    a = rstd * gamma.double()
    return a, beta.double() - m * a, rstd, m


def check_ratio(x64, G, ratio):
    mean, var = group_stats(x64, G)
    r = (mean.abs() / var.sqrt())
    if ratio == 0:
        assert float(r.max()) <= 1.0, float(r.max())
    else:
        # (a group of 2 channels x 64 pixels estimates its std from 128 values: +- 20 % around the ratio drawn)
        assert ratio * 0.75 <= float(r.min()) and float(r.max()) <= ratio * 1.3, (float(r.min()), float(r.max()))


def emulate_sums(x64, slab, chains, cross32):
    """(sum x, sum x^2) per (sample, channel) the way the kernels add: within each slab of `slab` rows, `chains` interleaved fp32
    running sums (one per thread: rows r, r + chains, ...), combined in fp32 (cross32: gn_partial_kernel, the conv epilogue) or in
    double (gn_fused_kernel), slabs added in double.  x64 (B, HW, C) -> two (B, C) fp64 arrays."""
    x = x64.numpy().astype(np.float32)
    B, HW, C = x.shape
    S = np.zeros((B, C)); Q = np.zeros((B, C))
    for r0 in range(0, HW, slab):
        blk = x[:, r0:r0 + slab]
        n = blk.shape[1]
        steps = -(-n // chains)
        pad = np.zeros((B, steps * chains, C), np.float32)
        pad[:, :n] = blk
        pad = pad.reshape(B, steps, chains, C)
        s = np.add.accumulate(pad, axis=1, dtype=np.float32)[:, -1]                       # sequential: one rounding per add
        q = np.add.accumulate(pad * pad, axis=1, dtype=np.float32)[:, -1]
        if cross32:
            s = np.add.accumulate(s, axis=1, dtype=np.float32)[:, -1]
            q = np.add.accumulate(q, axis=1, dtype=np.float32)[:, -1]
            S += s.astype(np.float64); Q += q.astype(np.float64)
        else:
            S += s.astype(np.float64).sum(1); Q += q.astype(np.float64).sum(1)
    return torch.from_numpy(S), torch.from_numpy(Q)


def emulated_ab(c, x64, gamma, beta, slab, chains, cross32):
    """the table a kernel of this summation order would give: group combine in double, rstd rounded to fp32, a and b in fp32"""
    B, HW, C = x64.shape
    G = c["G"]
    S, Q = emulate_sums(x64, slab, chains, cross32)
    n = float(HW * (C // G))
    mean = S.reshape(B, G, -1).sum(-1) / n
    var = (Q.reshape(B, G, -1).sum(-1) / n - mean * mean).clamp_min(0.0)
    rstd = (var + float(np.float32(c["eps"]))).rsqrt().float().repeat_interleave(C // G, 1)
    a = rstd * gamma
    b = beta - mean.float().repeat_interleave(C // G, 1) * a
    return a.double(), b.double()


def ab_errors(a, b, ref, gamma, beta):
    """(relative error of a, error of b in units of |beta| + |mean a|, relative error of rstd = a / gamma): worst element"""
    a_ref, b_ref, rstd, m = ref
    ea = float(((a - a_ref).abs() / a_ref.abs()).max())
    eb = float(((b - b_ref).abs() / (beta.double().abs() + (m * a_ref).abs())).max())
    er = float(((a / gamma.double() - rstd).abs() / rstd).max())
    return ea, eb, er


def assert_ab(tag, ratio, errs, y_rel=None):
    """the bounds of the module docstring for one table (and, at ratio 128, the output it gives)"""
    ea, eb, er = errs
    print("GN_CASE %-34s ratio=%-3d a=%.2e b=%.2e rstd=%.2e%s" % (tag, ratio, ea, eb, er, "" if y_rel is None else " y=%.2e" % y_rel))
    assert np.isfinite([ea, eb, er]).all()
    if ratio == 0:
        assert ea <= TOL_AB and eb <= TOL_AB, (tag, errs)
    elif ratio == 32:
        assert er <= TOL_RSTD32, (tag, errs)
    if y_rel is not None:
        assert np.isfinite(y_rel) and y_rel < (TOL_Y128 if ratio == 128 else TOL16), (tag, ratio, y_rel)


def assert_emulation(tag, ratio, errs):
    ea, eb, er = errs
    if ratio == 0:
        assert ea <= TOL_AB / 3 and eb <= TOL_AB / 3, (tag, errs)
    elif ratio == 32:
        assert er <= TOL_RSTD32 / 3, (tag, errs)


def rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def sent16(n):
    return torch.full((n,), SENT16, dtype=torch.int16, device="cuda")


def sent32(n):
    return torch.full((n,), SENT32, dtype=torch.int32, device="cuda")


def chains_of(c, L):
    """(slab, chains, cross32) of the emulation for a fused / stats case"""
    sc, slab, _ = gn_path(L, c["B"], c["HW"], c["C"], c["G"])
    if c["path"] == "fused":
        return c["HW"], 256 // (sc // 8), False
    return slab, partial_form(c["C"], slab)[0], True


# ------------------------------------------------------------------------------------------------------------------------------
# fused and statistics paths
# ------------------------------------------------------------------------------------------------------------------------------
def run_norm_case(c, L=None, gpu=True):
    L = L or lib()
    B, HW, C, G, eps = c["B"], c["HW"], c["C"], c["G"], c["eps"]
    sc, slab, nslab = gn_path(L, B, HW, C, G)
    if c["path"] == "fused":
        assert sc > 0 and sc % (C // G) == 0 and sc % 8 == 0 and C % sc == 0, sc          # the path the row claims
    else:
        assert slab == c["slab"] and nslab == -(-HW // slab)
    gamma, beta = affine(C, seed_of(c["id"]))
    em_slab, chains, cross32 = chains_of(c, L)
    out = {}
    for ratio in c.get("ratios", RATIOS):
        x16 = gn_input(c, ratio)
        if c.get("pair_in"):                                                 # a split pair: hi + lo carries 22 bits of a finer-grained x
            g = torch.Generator().manual_seed(seed_of(c["id"]) + 7)
            x32 = x16.float() * (1 + 2.0 ** -13 * torch.randn(x16.shape, generator=g))
            hi, lo = split16(x32)
            x64 = hi.double() + lo.double()
        else:
            hi, lo, x64 = x16, None, x16.double()
        check_ratio(x64, G, ratio)
        mean, var = group_stats(x64, G)
        ref = ab_from(mean, var, float(np.float32(eps)), gamma, beta, C)
        errs_emu = ab_errors(*emulated_ab(c, x64, gamma, beta, em_slab, chains, cross32), ref, gamma, beta)
        assert_emulation(c["id"], ratio, errs_emu)
        out[ratio] = dict(emu=errs_emu)
        if not gpu:
            continue
        y_ref = F.silu(x64 * ref[0][:, None, :] + ref[1][:, None, :])
        pad = c.get("ld_pad", 0)
        ld = (2 * C if lo is not None else C) + pad
        xin = torch.full((B, HW, ld), 77.0, dtype=torch.half)                # padding columns: a large value no sum may include
        xin[..., :C] = hi
        if lo is not None:
            xin[..., C:2 * C] = lo
        x_lo = C if lo is not None else 0
        gd, bd = gamma.cuda(), beta.cuda()
        if c.get("f32"):
            xd32, xd16 = x64.float().cuda(), None
            ld = C
        else:
            xd32, xd16 = None, xin.cuda()
        if c["path"] == "fused":
            # 1. the production form: 16-bit input, SiLU, fp16 output
            ybuf = sent16((B * HW + 8) * (C + 8))
            rc = L.gdf_op_groupnorm_split(P(xd16), x_lo, None, ld, B, HW, C, G, eps, P(gd), P(bd), 1, P(ybuf), C + 8, 0, None, stream())
            assert rc == 0, L.gdf_last_error().decode()
            # 2. the table: fp32 input (the same values), no SiLU, split output -> least squares per (sample, channel)
            x32d = x64.float().cuda()
            pbuf = sent16((B * HW + 8) * (2 * C + 8))
            rc = L.gdf_op_groupnorm_split(None, 0, P(x32d), C, B, HW, C, G, eps, P(gd), P(bd), 0, P(pbuf), 2 * C + 8, C, None, stream())
            assert rc == 0, L.gdf_last_error().decode()
            torch.cuda.synchronize()
            y2 = ybuf.cpu().view(B * HW + 8, C + 8)
            p2 = pbuf.cpu().view(B * HW + 8, 2 * C + 8)
            assert bool((y2[B * HW:] == SENT16).all()) and bool((y2[:, C:] == SENT16).all()), "written outside y"
            assert bool((p2[B * HW:] == SENT16).all()) and bool((p2[:, 2 * C:] == SENT16).all()), "written outside the y pair"
            y = y2[:B * HW, :C].contiguous().view(torch.half).view(B, HW, C)
            pr = p2[:B * HW, :2 * C].contiguous().view(torch.half).view(B, HW, 2 * C).double()
            yl = pr[..., :C] + pr[..., C:]
            xc = x64 - x64.mean(1, keepdim=True)
            a = (xc * (yl - yl.mean(1, keepdim=True))).sum(1) / (xc * xc).sum(1)
            b = yl.mean(1) - a * x64.mean(1)
        else:
            part = sent32(B * nslab * C * 2 + 64)
            abuf = sent32(B * C * 2 + 64)
            rc = L.gdf_op_gn_stats(P(xd16), x_lo, P(xd32), ld, B, HW, C, G, eps, P(gd), P(bd), P(part), P(abuf), stream())
            assert rc == 0, L.gdf_last_error().decode()
            wy = 2 * C if c.get("pair_out") else C
            ybuf = sent16((B * HW + 8) * (wy + 8))
            rc = L.gdf_op_gn_apply(P(xd16), x_lo, P(xd32), ld, B, HW, C, P(abuf), 1, P(ybuf), wy + 8, C if c.get("pair_out") else 0, stream())
            assert rc == 0, L.gdf_last_error().decode()
            torch.cuda.synchronize()
            assert bool((part[B * nslab * C * 2:] == SENT32).all()) and bool((abuf[B * C * 2:] == SENT32).all()), "written outside the tables"
            assert bool((part[:B * nslab * C * 2] != SENT32).all()), "a slab was not written"
            y2 = ybuf.cpu().view(B * HW + 8, wy + 8)
            assert bool((y2[B * HW:] == SENT16).all()) and bool((y2[:, wy:] == SENT16).all()), "written outside y"
            t = abuf[:B * C * 2].view(torch.float32).cpu().double().view(B, C, 2)
            a, b = t[..., 0], t[..., 1]
            y = y2[:B * HW, :wy].contiguous().view(torch.half).view(B, HW, wy)
            if c.get("pair_out"):
                pair = y[..., :C].double() + y[..., C:].double()
                assert rel(pair, y_ref) < rel(y[..., :C], y_ref)                        # the lo half adds accuracy
                if ratio == 0:
                    assert rel(pair, y_ref) < 1e-5                                        # fp32 arithmetic (__expf: 2 ulp) on a 2e-6 table
                y = y[..., :C]
        assert bool(torch.isfinite(y.float()).all())
        errs = ab_errors(a, b, ref, gamma, beta)
        y_rel = rel(y, y_ref)
        assert_ab(c["id"], ratio, errs, y_rel)
        out[ratio].update(gpu=errs, y=y_rel)
    return out


NORM_CASES = [c for c in CASES if c["path"] != "conv"]
CONV_CASES = [c for c in CASES if c["path"] == "conv"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", NORM_CASES, ids=[c["id"] for c in NORM_CASES])
def test_groupnorm_table(c):
    run_norm_case(c)


# ------------------------------------------------------------------------------------------------------------------------------
# statistics from the conv epilogue
# ------------------------------------------------------------------------------------------------------------------------------
def conv_reference(c, ratio):
    """inputs (fp16-rounded) and the fp64 epilogue chain: v0 = conv + bias + temb[sample], v = v0 + res -> dict"""
    B, H, W, Cin, N = c["B"], c["H"], c["W"], c["Cin"], c["C"]
    stride, ups = c.get("stride", 1), c.get("ups", 0)
    g = torch.Generator().manual_seed(seed_of(c["id"]))
    cin = 4 if c.get("conv_in") else Cin
    x = torch.randn(B, cin, H, W, generator=g).half()
    w = (torch.randn(N, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    bias = (0.5 + 0.15 * torch.randn(N, generator=g)).float()                           # group means away from 0: b's bound is relative to |mean a|
    xi = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
    cols = F.unfold(xi, 3, padding=1, stride=stride)                                       # (B, cin * 9, OH * OW)
    OH, OW = (xi.shape[2] - 1) // stride + 1, (xi.shape[3] - 1) // stride + 1
    v0 = (w.double().reshape(N, -1) @ cols).permute(0, 2, 1)                               # (B, OH * OW, N)
    r = dict(x=x, w=w, OH=OH, OW=OW, HW=OH * OW, M=B * OH * OW)
    if c.get("conv_in"):
        temb = res = None
    else:
        temb = (0.15 * torch.randn(B, N, generator=g)).float()
        res = torch.randn(B, OH * OW, N, generator=g).float()
    sd = float((v0 + bias.double() + (res.double() if res is not None else 0.0)).std())
    if ratio:                                                                              # the offset comes in through the bias
        bias = (bias + ratio * sd).float()
    v0 = v0 + bias.double() + (temb.double()[:, None, :] if temb is not None else 0.0)
    v = v0 + (res.double() if res is not None else 0.0)
    r.update(bias=bias, temb=temb, res=res, v0=v0, v=v * (c.get("scale") or 1.0))
    return r


def slab_sums(v, slab):
    """v (B, HW, N) fp64 -> (M / slab, N) sums and sums of squares over consecutive row slabs of the (M, N) matrix"""
    N = v.shape[-1]
    t = v.reshape(-1, slab, N)
    return t.sum(1), (t * t).sum(1)


def launch_conv(L, c, r, gpart_slabs, sentinel_out=True):
    """one gdf_op_conv3x3_gn / gdf_op_conv_in_gn launch into sentinel-filled buffers -> rc and the device buffers"""
    B, H, W, N, M = c["B"], c["H"], c["W"], c["C"], r["M"]
    o16 = sent16((M + 8) * N)
    aux = sent16((M + 8) * N)
    part = sent32((gpart_slabs + 2) * N * 2)
    scale = c.get("scale", 0.0)
    if c.get("conv_in"):
        xd, wd, bd = r["x"].cuda(), r["w"].cuda(), r["bias"].cuda()
        scratch = torch.zeros(B * H * W * 16 + N * 256, dtype=torch.uint8, device="cuda")
        rc = L.gdf_op_conv_in_gn(P(xd), B, 4, H, W, P(wd), P(bd), N, P(o16), P(scratch), scale, P(part), stream())
    else:
        Cin = c["Cin"]
        xd = r["x"].permute(0, 2, 3, 1).contiguous().cuda()
        ws, bd, td, rd = r["w"].cuda(), r["bias"].cuda(), r["temb"].cuda(), r["res"].cuda()
        wd = torch.empty(N, 9 * Cin, dtype=torch.half, device="cuda")
        assert L.gdf_op_relayout_conv3(P(ws), P(wd), N, Cin, stream()) == 0
        rc = L.gdf_op_conv3x3_gn(P(xd), Cin, B, H, W, Cin, P(wd), N, P(bd), P(td), c.get("stride", 1), c.get("ups", 0), P(rd), P(aux),
                                 P(o16), None, c["variant"] << 8, scale, P(part), stream())
    torch.cuda.synchronize()
    return rc, o16, aux, part


def run_conv_case(c, L=None, gpu=True):
    L = L or lib()
    B, H, W, N, G, eps = c["B"], c["H"], c["W"], c["C"], c["G"], c["eps"]
    name, slab = conv_info(L, B, H, W, 4 if c.get("conv_in") else c["Cin"], N, c.get("stride", 1), c.get("ups", 0), c["variant"])
    assert name == c["kernel"], name                                                        # the instantiation the row claims
    assert slab == (128 if c["kernel"] == K932 else 64)
    gamma, beta = affine(N, seed_of(c["id"]))
    out = {}
    for ratio in c.get("ratios", RATIOS):
        r = conv_reference(c, ratio)
        M, HW = r["M"], r["HW"]
        assert M % slab == 0 and HW % slab == 0
        nslab = HW // slab
        v = r["v"]
        check_ratio(v, G, ratio)
        mean, var = group_stats(v, G)
        ref = ab_from(mean, var, float(np.float32(eps)), gamma, beta, N)
        # the epilogue: a lane adds the rows it stores (every 8th of the wave tile for 64-column wave tiles), the lanes are combined in fp32
        errs_emu = ab_errors(*emulated_ab(c, v, gamma, beta, slab, 8, True), ref, gamma, beta)
        assert_emulation(c["id"], ratio, errs_emu)
        out[ratio] = dict(emu=errs_emu)
        if not gpu:
            continue
        rc, o16, aux, part = launch_conv(L, c, r, M // slab)
        assert rc == 0, L.gdf_last_error().decode()
        assert bool((o16[M * N:] == SENT16).all()) and bool((part[M // slab * N * 2:] == SENT32).all()), "written outside the result"
        got16 = o16[:M * N].view(torch.half).cpu().view(B, HW, N)
        assert rel(got16, v) < TOL16
        if not c.get("conv_in"):
            assert bool((aux[M * N:] == SENT16).all())
            assert rel(aux[:M * N].view(torch.half).cpu().view(B, HW, N), r["v0"]) < TOL16
        # per-slab sums of exactly that slab's rows
        ps = part[:M // slab * N * 2].view(torch.float32).cpu().double().view(M // slab, N, 2)
        s_ref, q_ref = slab_sums(v, slab)
        es = float(((ps[..., 0] - s_ref).norm(dim=1) / s_ref.norm(dim=1)).max())
        eq = float(((ps[..., 1] - q_ref).norm(dim=1) / q_ref.norm(dim=1)).max())
        print("GN_CASE %-34s ratio=%-3d slab sums: sum=%.2e squares=%.2e (bound %.0e), %d slabs of %d rows" % (c["id"], ratio, es, eq, TOL32, M // slab, slab))
        assert es < TOL32 and eq < TOL32, (es, eq)
        # the chain: finalize on those sums, apply on the stored fp16 image
        abuf = sent32(B * N * 2 + 64)
        fold_n = L.gdf_op_gn_fold_floats(B, nslab, N)
        fold = sent32(fold_n + 64) if fold_n else None
        gd, bd = gamma.cuda(), beta.cuda()
        rc = L.gdf_op_gn_finalize(P(part), nslab, B, HW, N, G, eps, P(gd), P(bd), P(abuf), P(fold), stream())
        assert rc == 0, L.gdf_last_error().decode()
        ybuf = sent16((M + 8) * N)
        rc = L.gdf_op_gn_apply(P(o16), 0, None, N, B, HW, N, P(abuf), 1, P(ybuf), N, 0, stream())
        assert rc == 0, L.gdf_last_error().decode()
        torch.cuda.synchronize()
        assert bool((abuf[B * N * 2:] == SENT32).all()) and bool((ybuf[M * N:] == SENT16).all())
        t = abuf[:B * N * 2].view(torch.float32).cpu().double().view(B, N, 2)
        errs = ab_errors(t[..., 0], t[..., 1], ref, gamma, beta)
        y = ybuf[:M * N].view(torch.half).cpu().view(B, HW, N)
        # benign: against fp64 silu(group_norm(fp64 conv output)).  Offset runs: fp16 storage of the image alone moves the normalised value by
        # ratio x 2^-11 (1.6 % at 32), so the output is compared with the exact table applied to the stored image: what is left is the table's error
        y_ref = F.silu((v if ratio == 0 else got16.double()) * ref[0][:, None, :] + ref[1][:, None, :])
        y_rel = rel(y, y_ref)
        assert_ab(c["id"], ratio, errs, y_rel)
        out[ratio].update(gpu=errs, sums=(es, eq), y=y_rel)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", CONV_CASES, ids=[c["id"] for c in CONV_CASES])
def test_conv_epilogue_statistics(c):
    run_conv_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("id,variant,B,H,W,Cout", [("m36-128", 128, 1, 6, 6, 64), ("m36-auto", 0, 1, 6, 6, 64), ("m100-826", 826, 1, 10, 10, 256),
                                                   ("m192-932", 932, 3, 8, 8, 320)])
def test_conv_epilogue_statistics_refused_shapes(id, variant, B, H, W, Cout):
    """M % 64 != 0, and M % 128 != 0 on the 256x320 tile: no kernel name, an error, nothing written"""
    L = lib()
    c = conv("refused-" + id, None, variant, B, H, W, Cout)
    assert conv_info(L, B, H, W, 64, Cout, 1, 0, variant) == (None, 0)
    r = conv_reference(c, 0)
    rc, o16, aux, part = launch_conv(L, c, r, -(-r["M"] // 64))
    assert rc != 0 and b"conv3x3_gn" in L.gdf_last_error()
    assert bool((o16 == SENT16).all()) and bool((aux == SENT16).all()) and bool((part == SENT32).all())


# ------------------------------------------------------------------------------------------------------------------------------
# fold
# ------------------------------------------------------------------------------------------------------------------------------
def fold_inputs(nslab, C, B=2, rows=64):
    """synthetic per-slab sums of `rows` values of mean mu_c and std 2 per channel, as the fp32 an epilogue would store"""
    g = torch.Generator().manual_seed(nslab * 4099 + C)
    mu = 0.5 + 0.2 * torch.randn(1, 1, C, generator=g)
    s = rows * (mu + 0.25 * torch.randn(B, nslab, C, generator=g))
    q = s * s / rows + rows * 4.0 * (1 + 0.2 * torch.rand(B, nslab, C, generator=g))
    return torch.stack([s, q], -1).float()                                                  # (B, nslab, C, 2)


def fold_reference(part, G, eps, gamma, beta, rows=64):
    B, nslab, C, _ = part.shape
    tot = part.double().sum(1)                                                              # (B, C, 2)
    n = float(nslab * rows * (C // G))
    mean = tot[..., 0].reshape(B, G, -1).sum(-1) / n
    var = tot[..., 1].reshape(B, G, -1).sum(-1) / n - mean * mean
    return ab_from(mean, var, float(np.float32(eps)), gamma, beta, C)


@pytest.mark.gpu
@pytest.mark.parametrize("nslab,C", FOLD_CASES)
def test_finalize_fold(nslab, C):
    L = lib()
    B, G, eps = 2, 32, 1e-5
    want_fold = fold_shape(nslab, C)
    part = fold_inputs(nslab, C)
    gamma, beta = affine(C, nslab + C)
    ref = fold_reference(part, G, eps, gamma, beta)
    n_fold = L.gdf_op_gn_fold_floats(B, nslab, C)
    assert (n_fold > 0) == (nslab > 256)
    pd, gd, bd = part.cuda(), gamma.cuda(), beta.cuda()
    tabs = []
    for use_fold in (True, True, False):
        abuf = sent32(B * C * 2 + 64)
        fold = sent32(n_fold + 64) if (use_fold and n_fold) else None
        rc = L.gdf_op_gn_finalize(P(pd), nslab, B, nslab * 64, C, G, eps, P(gd), P(bd), P(abuf), P(fold), stream())
        assert rc == 0, L.gdf_last_error().decode()
        torch.cuda.synchronize()
        assert bool((abuf[B * C * 2:] == SENT32).all())
        if fold is not None:
            per = -(-nslab // 128)
            used = B * (-(-nslab // per)) * C * 2 if want_fold else 0
            assert bool((fold[used:] == SENT32).all()), "written outside the fold scratch"
            assert bool((fold[:used] != SENT32).all()), "the fold did not run (or left a slab out)"
        tabs.append(abuf[:B * C * 2].clone())
    assert torch.equal(tabs[0], tabs[1])                                                    # fixed order: two launches bit-identical
    t = [x.view(torch.float32).cpu().double().view(B, C, 2) for x in (tabs[0], tabs[2])]
    for name, x in zip(("fold", "gather"), t):
        assert_ab("fold-n%d-c%d-%s" % (nslab, C, name), 0, ab_errors(x[..., 0], x[..., 1], ref, gamma, beta))
    d = float(((t[0] - t[1]).abs() / (t[1].abs() + beta.double().abs()[None, :, None])).max())
    assert d <= 1e-6, d
    assert torch.equal(part, pd.cpu())                                                      # the fold reads its input only


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm template widths
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("R,C", LN_CASES)
@pytest.mark.parametrize("f32", [0, 1])
def test_layernorm_template_boundaries(R, C, f32):
    L = lib()
    ld = C + 24
    g = torch.Generator().manual_seed(R * 10007 + C)
    x = (3.0 * torch.randn(R, ld, generator=g) + 1.0).half()
    x[:, C:] = 500.0                                                                        # columns beyond C: no statistic may include them
    gamma, beta = affine(C, C)
    ref = F.layer_norm(x[:, :C].double(), (C,), gamma.double(), beta.double(), 1e-5)
    ybuf = sent16((R + 8) * C)
    xd = x.float().cuda() if f32 else x.cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    rc = L.gdf_op_layernorm(None if f32 else P(xd), P(xd) if f32 else None, ld, R, C, 1e-5, P(gd), P(bd), P(ybuf), stream())
    assert rc == 0, L.gdf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((ybuf[R * C:] == SENT16).all())
    y = ybuf[:R * C].view(torch.half).cpu().view(R, C).double()
    row = float(((y - ref).norm(dim=1) / ref.norm(dim=1)).max())
    print("LN_CASE R=%d C=%d f32=%d tensor=%.2e worst row=%.2e" % (R, C, f32, rel(y, ref), row))
    assert rel(y, ref) < TOL16 and row < TOL16


@pytest.mark.gpu
def test_layernorm_rejects_rows_wider_than_the_templates():
    L = lib()
    R, C = 5, 2056
    x = torch.zeros(R, C, dtype=torch.half, device="cuda")
    gb = torch.ones(C, device="cuda")
    ybuf = sent16(R * C)
    rc = L.gdf_op_layernorm(P(x), None, C, R, C, 1e-5, P(gb), P(gb), P(ybuf), stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"layernorm" in L.gdf_last_error()
    assert bool((ybuf == SENT16).all())
