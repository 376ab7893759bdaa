"""Kernel-level parity of every GEMM / 3x3-conv kernel launch_gemm can pick (-m gpu), through gdf_op_gemm_ex (and gdf_op_conv_in /
gdf_op_gemm_mx for the plain conv_in rows and the fp8 form, which keep their own entry points; the conv_in of a "precise" plan, whose output is a
(hi, lo) pair, runs through gdf_op_gemm_ex on operands packed as gdf_op_conv_in packs them).

CASES is the map from kernel instantiation to the test that runs it; tests/test_gemm_dispatch_cpu.py asserts (without a GPU) that every
instantiation a sweep of legal arguments reaches has a row here.  To add a case for a new instantiation: add a row whose arguments make
launch_gemm choose it (usually `variant`) and write the symbol into `kernel` (GK / SK / DK / DSK / MX below).

Every case draws seeded inputs, rounds them to the element type, computes the op in fp64 on the CPU from the rounded values
(F.conv2d in double for convs, explicit F.pad / F.interpolate for pad0 / ups) and asserts
  1. gdf_op_gemm_kernel(args) == the `kernel` of the row,
  2. whole-tensor relative L2: fp16 outputs 1e-3, fp32 outputs 2e-4, split (hi, lo) pairs 3e-6 (bf16: x 8),
  3. the same bounds per 16-row x 16-column block of the output, so that one wrong MFMA fragment fails,
  4. nothing is written outside the result: sentinel columns right of N, sentinel rows below M, a sentinel gap between the hi and lo halves
     of a pair and between the slabs of a grouped launch (0x5A5A),
  5. nothing outside the operands is used: A and W sit inside larger allocations whose other rows / columns hold 1e4.
Before it looks at the GPU result a case asserts that a CPU emulation of the contract (fp32 accumulation of the rounded operands, fp32 epilogue,
one rounding to the output type) is under bound / 3 per block: the inputs (bias offset), not the bounds, are what gets changed if that fails.
Convs have K = 9 Cin >= 9 K-tiles, so their K ladder is Cin = 64 / 192 (9 / 27 K-tiles) instead of 1 / 3 / 11 K-tiles.
"""
import ctypes
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from ops_binding import GemmArgs, P, lib, ok, stream

TOL16, TOL32, TOL_PAIR, BF_FACTOR = 1e-3, 2e-4, 3e-6, 8.0
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
POISON = 1e4                 # rows after A / W, columns right of K: large, finite; the kernel must never use them
F16_MAX = 65504.0


def _t(v):
    return "true" if v else "false"


def GK(mode, bm, bn, st, geglu=False):
    return "gemm_kernel<%d, %d, %d, %d, %s>" % (mode, bm, bn, st, _t(geglu))


def SK(mode, bm, bn, st, geglu=False):
    return "gemm_split_kernel<%d, %d, %d, %d, %s>" % (mode, bm, bn, st, _t(geglu))


def DK(bm, bn, st, bf=False, qkn=False):
    return "gemm_dit_kernel<%d, %d, %d, %s, %s>" % (bm, bn, st, _t(bf), _t(qkn))


def DSK(bm, bn, st, qkn=False):
    return "gemm_dit_split_kernel<%d, %d, %d, true, %s>" % (bm, bn, st, _t(qkn))


MX = "gemm_mx_kernel<256, 256, 8>"
# tile (rows, columns, stages) of a forced `variant`
TILE = {128: (128, 128, 2), 160: (128, 160, 2), 256: (256, 128, 3), 320: (256, 320, 2), 932: (256, 320, 9), 826: (256, 256, 8),
        825: (256, 256, 8)}
DTILE = {128: (128, 128, 2), 2128: (256, 128, 3), 1256: (256, 256, 2), 8256: (256, 256, 8)}


def dense(id, kernel, M, N, K, **kw):
    return dict(id=id, kernel=kernel, form="dense", M=M, N=N, K=K, **kw)


def conv(id, kernel, B, H, W, Cin, N, **kw):
    return dict(id=id, kernel=kernel, form="conv", B=B, H=H, W=W, Cin=Cin, N=N, **kw)


def _hw(M):
    """an image of exactly M pixels (M = BM + 72: 200 or 328)"""
    return {200: (10, 20), 328: (8, 41)}[M]


CASES = []


def _tiles():
    """a. every instantiation x ragged M / N (M = BM + 72, N = BN + 24 or the next legal multiple) x the K ladder"""
    rows = []
    for k in (64, 192, 704):                                                            # 1, 3, 11 K-tiles
        for v in (128, 160, 256, 320, 932):
            bm, bn, st = TILE[v]
            rows.append(dense("tile-dense-%dx%d-s%d-k%d" % (bm, bn, st, k), GK(0, bm, bn, st), bm + 72, bn + 24, k, variant=v, res="f32"))
        for n in (4, 20):
            rows.append(dense("tile-dense-128x16-n%d-k%d" % (n, k), GK(0, 128, 16, 2), 200, n, k, bn=16))
        for v in (128, 256, 320, 825):
            bm, bn, st = TILE[v]
            rows.append(dense("tile-geglu-%dx%d-s%d-k%d" % (bm, bn, st, k), GK(0, bm, bn, st, True), bm + 72, bn + 32, k, variant=v, geglu=True,
                              o32=False, bias_off=3.0, gate_off=2.0))
        for v in (128, 160, 932):
            bm, bn, st = TILE[v]
            rows.append(dense("tile-split-dense-%dx%d-s%d-k%d" % (bm, bn, st, k), SK(0, bm, bn, st), bm + 72, bn + 24, k, variant=v, a_pair=True,
                              o_pair=True, bias_off=4.0))
        for v in (128, 825):
            bm, bn, st = TILE[v]
            rows.append(dense("tile-split-geglu-%dx%d-s%d-k%d" % (bm, bn, st, k), SK(0, bm, bn, st, True), bm + 72, bn + 32, k, variant=v, geglu=True,
                              a_pair=True, o_pair=True, o32=False, bias_off=4.0, gate_off=2.0))
        for bf in (0, 1):
            for v in (128, 2128, 1256, 8256):
                bm, bn, st = DTILE[v]
                rows.append(dense("tile-dit-%dx%d-s%d-%s-k%d" % (bm, bn, st, "bf16" if bf else "f16", k), DK(bm, bn, st, bf), bm + 72, bn + 24, k,
                                  variant=v, dit=1, bf16=bf, res="f32"))
            for v in (1256, 8256):
                bm, bn, st = DTILE[v]
                rows.append(dense("tile-dit-qkn-%dx%d-s%d-%s-k%d" % (bm, bn, st, "bf16" if bf else "f16", k), DK(bm, bn, st, bf, True), bm + 72, 384, k,
                                  variant=v, dit=1, bf16=bf, qkn=True, o32=False))
        for v, q in ((128, False), (8256, False), (8256, True)):
            bm, bn, st = DTILE[v]
            rows.append(dense("tile-dit-split-%dx%d%s-k%d" % (bm, bn, "-qkn" if q else "", k), DSK(bm, bn, st, q), bm + 72, 384 if q else bn + 24, k,
                              variant=v, dit=1, bf16=1, a_pair=True, o_pair=True, qkn=q, o32=False, bias_off=0.0 if q else 4.0))
    for cin in (64, 192):                                                               # 9, 27 K-tiles
        for v in (128, 160, 256, 320, 932, 826):
            bm, bn, st = TILE[v]
            h, w = _hw(bm + 72)
            rows.append(conv("tile-conv-%dx%d-s%d-c%d" % (bm, bn, st, cin), GK(1, bm, bn, st), 1, h, w, cin, bn + 24, variant=v, res="f32"))
        for n in (4, 20):
            rows.append(conv("tile-conv-128x16-n%d-c%d" % (n, cin), GK(1, 128, 16, 2), 1, 10, 20, cin, n, bn=16))
        for v in (128, 160, 932):
            bm, bn, st = TILE[v]
            h, w = _hw(bm + 72)
            rows.append(conv("tile-split-conv-%dx%d-s%d-c%d" % (bm, bn, st, cin), SK(1, bm, bn, st), 1, h, w, cin, bn + 24, variant=v, a_pair=True,
                             o_pair=True, bias_off=4.0))
        for n in (4, 20):
            rows.append(conv("tile-split-conv-128x16-n%d-c%d" % (n, cin), SK(1, 128, 16, 2), 1, 10, 20, cin, n, bn=16, a_pair=True))
    # conv_in and the fp8 GEMM keep their entry points (gdf_op_conv_in, gdf_op_gemm_mx); the name query covers them
    rows.append(dict(id="tile-conv-in-128x128", kernel=GK(2, 128, 128, 2), form="conv_in", B=1, H=10, W=20, Cin=4, N=152))
    rows.append(dict(id="tile-conv-in-128x160", kernel=GK(2, 128, 160, 2), form="conv_in", B=2, H=10, W=20, Cin=4, N=160))
    # the conv_in form through the complete launch: sentinel columns (ldo16 > N), and the pair output of a "precise" plan's conv_in
    # (gemm_split_kernel<2, ...>: the operand is plain, o16_lo alone selects it).  N = 160 takes the 128x160 tile by itself, `variant` gives it a ragged N
    cin_ex = lambda id, kernel, B, N, **kw: dict(id=id, kernel=kernel, form="conv_in_ex", B=B, H=10, W=20, Cin=4, N=N, **dict(dict(o32=False), **kw))
    rows += [
        cin_ex("tile-conv-in-ex-128x128", GK(2, 128, 128, 2), 1, 152),
        cin_ex("tile-conv-in-ex-128x160-n184", GK(2, 128, 160, 2), 1, 184, variant=160),
        cin_ex("tile-split-conv-in-128x128", SK(2, 128, 128, 2), 1, 152, o_pair=True, bias_off=4.0),
        cin_ex("tile-split-conv-in-128x160-n184", SK(2, 128, 160, 2), 1, 184, variant=160, o_pair=True, bias_off=4.0),
        cin_ex("tile-split-conv-in-128x160-n160", SK(2, 128, 160, 2), 2, 160, o_pair=True, bias_off=4.0),
        cin_ex("tile-split-conv-in-128x128-rowvec-out32", SK(2, 128, 128, 2), 3, 152, o_pair=True, bias_off=4.0, rowvec=200, o32=True),
    ]
    for k in (128, 384, 1408):
        rows.append(dict(id="tile-mx-k%d" % k, kernel=MX, form="mx", M=328, N=280, K=k))
    return rows


def _persistent():
    """b. persistent grids (more tiles than workgroups) and the tile order; K = 64 (one K-tile): memory-sized"""
    rows = [
        dense("persist-dense-932-17x16", GK(0, 256, 320, 9), 4168, 5096, 64, variant=932, o32=False),
        dense("persist-geglu-825-17x20", GK(0, 256, 256, 8, True), 4168, 5088, 64, variant=825, geglu=True, o32=False, bias_off=3.0, gate_off=2.0),
        conv("persist-conv-826-17x16", GK(1, 256, 256, 8), 1, 64, 65, 64, 4072, variant=826, o32=False),
        conv("persist-conv-932-17x16", GK(1, 256, 320, 9), 1, 64, 65, 64, 5096, variant=932, o32=False),
        dense("persist-dit-8256-17x16-f16", DK(256, 256, 8), 4168, 4072, 64, variant=8256, dit=1, o32=False),
        dense("persist-dit-8256-17x16-bf16", DK(256, 256, 8, True), 4168, 4072, 64, variant=8256, dit=1, bf16=1, o32=False),
        dict(id="persist-mx-17x16", kernel=MX, form="mx", M=4168, N=4072, K=128),
        # (launch_t walks tiles persistently in the 8-stage kernels only: the 256x320 8-phase rows above and below launch one workgroup per tile)
        # 64 workgroups walk 72 tiles: all take a first tile, 8 a second
        dense("persist-dit-8256-cus64-6x12", DK(256, 256, 8), 1464, 3064, 64, variant=8256, dit=1, cus=64, o32=False),
        conv("persist-conv-826-cus64-6x12", GK(1, 256, 256, 8), 1, 24, 61, 64, 3064, variant=826, cus=64, o32=False),
        dense("persist-dense-932-cus64-6x12", GK(0, 256, 320, 9), 1464, 3824, 64, variant=932, cus=64, o32=False),
        conv("persist-conv-932-cus64-6x12", GK(1, 256, 320, 9), 1, 24, 61, 64, 3824, variant=932, cus=64, o32=False),
        # super-block order against the linear order (no_superblock = 1): bit-identical.  launch_t takes the 2-D order only from 8 super-blocks
        # of (32 | 64 | cus / 8 workgroups) up, so the first three shapes (4 super-blocks) run linear either way and the next three engage it
        dense("order-256row-16x8", GK(0, 256, 320, 9), 4096, 2560, 64, variant=932, sb=True, o32=False),
        dense("order-128row-32x8", GK(0, 128, 128, 2), 4096, 1024, 64, variant=128, sb=True, o32=False),
        dense("order-256row-cus64-4x8", GK(0, 256, 320, 9), 1024, 2560, 64, variant=932, cus=64, sb=True, o32=False),
        dense("order-256row-16x16", GK(0, 256, 320, 2), 4096, 5120, 64, variant=320, sb=True, o32=False),
        dense("order-128row-32x16", GK(0, 128, 128, 2), 4096, 2048, 64, variant=128, sb=True, o32=False),
        dense("order-256row-cus64-8x8", GK(0, 256, 320, 9), 2048, 2560, 64, variant=932, cus=64, sb=True, o32=False),
        dense("order-256row-17x16-fallback", GK(0, 256, 320, 2), 4168, 5120, 64, variant=320, sb=True, o32=False),   # 17 % 8: linear order
    ]
    return rows


def _epilogues():
    """c. epilogue forms on one ring tile and one 8-phase tile, ragged M and N"""
    rows = []
    for tag, v, M, N in (("ring", 128, 200, 152), ("8ph", 932, 328, 344)):
        bm, bn, st = TILE[v]
        k = GK(0, bm, bn, st)
        d = lambda id, **kw: dense("epi-%s-%s" % (tag, id), kw.pop("kernel", k), M, N, 192, variant=v, **kw)
        rows += [
            d("bias-only"),
            d("nobias-out16-only", bias=False, o32=False),
            d("out32-only", o16=False),
            d("rowvec-rps100", rowvec=100),
            d("rowvec-res32", rowvec=100, res="f32"),
            d("aux-res32", aux=True, res="f32"),
            d("aux-res16", aux=True, res="f16"),
            d("wide-lds", aux=True, res="f32", wide=True),
            d("wide-lds-res16", res="f16", wide=True, rowvec=100),
            d("acc-scale", scale=True, bias_off=8.0, a_off=1.5),
        ]
        cv = GK(1, bm, bn, st)
        h, w = _hw(M)
        rows += [
            conv("epi-%s-conv-rowvec-rps100" % tag, cv, 1, h, w, 64, N, variant=v, rowvec=100),
            conv("epi-%s-conv-aux-res32" % tag, cv, 1, h, w, 64, N, variant=v, aux=True, res="f32"),
            conv("epi-%s-conv-acc-scale" % tag, cv, 1, h, w, 64, N, variant=v, scale=True, bias_off=8.0, a_off=1.5),
        ]
    for tag, v, M, N in (("ring", 128, 200, 152), ("8ph", 8256, 328, 280)):
        bm, bn, st = DTILE[v]
        for bf in (0, 1):
            k = DK(bm, bn, st, bf)
            e = "bf16" if bf else "f16"
            d = lambda id, **kw: dense("epi-dit-%s-%s-%s" % (tag, e, id), k, M, N, 192, variant=v, dit=1, bf16=bf, **kw)
            rows += [
                d("gelu", act=1),
                d("gate-res32-aux", rowvec=100, rv_mul=1, res="f32", aux=True),          # aux16 holds the projection BEFORE the gate
                d("shift", rowvec=100, rv_mul=0),
                d("gate-seg-rows", rowvec=40, rv_mul=1, rv_seg=(80, 62), res="f32"),     # 2 x 40 text rows, then 62-row image samples
                d("rv-tok", rowvec=100, rv_tok=1, res="f32"),
                d("acc-scale", scale=True, bias_off=8.0, a_off=1.5),
            ]
        k = DK(bm, bn, st, True)
        rows.append(dense("epi-dit-%s-bf16-out-f16-saturates" % tag, k, M, N, 192, variant=v, dit=1, bf16=1, out_f16=1, aux=True, spikes=True))
    return rows


def _geometry():
    """d. conv geometry; Cout = 64 takes the 128x128 tile, Cout = 160 the 128x160 tile"""
    rows = []
    for n, k in ((64, GK(1, 128, 128, 2)), (160, GK(1, 128, 160, 2))):
        c = lambda id, B, H, W, **kw: conv("geo-n%d-%s" % (n, id), k, B, H, W, kw.pop("Cin", 64), n, **kw)
        rows += [c("%dx%d-s%d" % (h, w, s), 2, h, w, stride=s) for (h, w) in ((7, 9), (5, 3), (2, 2)) for s in (1, 2)]
        rows += [
            c("ups-3x5", 2, 3, 5, ups=1),
            c("pad0-8x6", 2, 8, 6, stride=2, pad0=1),
            c("pad0-7x9", 2, 7, 9, stride=2, pad0=1),
            c("b3-63px-rowvec", 3, 7, 9, rowvec=63),
            c("wide-ld", 2, 7, 9, wide=True),
            c("cin192", 2, 7, 9, Cin=192),
        ]
    return rows


def _grouped():
    """e. grouped launch: 3 weight matrices over one A (two samples of 77 text tokens)"""
    return [
        dense("batch3-n320", GK(0, 128, 128, 2), 154, 320, 128, batch=3, bias=False, o32=False),
        dense("batch3-n640", GK(0, 128, 128, 2), 154, 640, 128, batch=3, bias=False, o32=False),
        dense("batch3-n320-pair", SK(0, 128, 128, 2), 154, 320, 128, batch=3, o32=False, o_pair=True, bias_off=4.0),
        dense("batch3-n640-pair", SK(0, 128, 128, 2), 154, 640, 128, batch=3, o32=False, o_pair=True, bias_off=4.0),
    ]


def _splitk():
    """f. split-K through gdf_op_gemm_ex: N = 256 takes the 128x128 tile, N = 320 the 128x160 tile"""
    rows = []
    for n, bn in ((256, 128), (320, 160)):
        k, ks, cv = GK(0, 128, bn, 2), SK(0, 128, bn, 2), GK(1, 128, bn, 2)
        d = lambda id, K=448, S=3, **kw: dense("splitk-n%d-%s" % (n, id), kw.pop("kernel", k), 200, n, K, splitk=S, **kw)
        rows += [
            d("7tiles-by3", res="f32", aux=True),
            d("clamped", K=128, S=5, res="f32"),
            d("rowvec-res16", rowvec=100, res="f16", aux=True),
            d("pair", kernel=ks, o_pair=True, bias_off=4.0),
            d("acc-scale", scale=True, bias_off=8.0, a_off=1.5),
            d("wide-lds", wide=True, rowvec=100, res="f32", aux=True),                     # ldres, ldrv, ldaux, ldo16, ldo32 > N, a column offset
            d("wide-lds-res16-pair", kernel=ks, wide=True, res="f16", o_pair=True, bias_off=4.0),
            conv("splitk-n%d-conv-9tiles-by4" % n, cv, 1, 10, 20, 64, n, splitk=4, rowvec=100, res="f32", aux=True),
            conv("splitk-n%d-conv-clamped" % n, cv, 1, 10, 20, 64, n, splitk=12, res="f32"),
        ]
    return rows


def is_conv(c):
    return c["form"] in ("conv", "conv_in_ex")


CASES = _tiles() + _persistent() + _epilogues() + _geometry() + _grouped() + _splitk()


# ------------------------------------------------------------------------------------------------------------------------------
# layout of a case: sizes, leading dimensions, offsets
# ------------------------------------------------------------------------------------------------------------------------------
def up8(n):
    return (n + 7) // 8 * 8


def layout(c):
    y = dict()
    if c["form"] in ("conv", "conv_in", "conv_in_ex"):
        ups, s = c.get("ups", 0), c.get("stride", 1)
        IH, IW = (2 * c["H"], 2 * c["W"]) if ups else (c["H"], c["W"])
        y["OH"], y["OW"] = (IH - 1) // s + 1, (IW - 1) // s + 1
        y["M"], y["Kw"] = c["B"] * y["OH"] * y["OW"], c["Cin"]
    else:
        y["M"], y["Kw"] = c["M"], c["K"]
    N = c["N"]
    y["N"], y["Nout"] = N, N // 2 if c.get("geglu") else N
    kw = y["Kw"]
    y["a_off"] = 32 if c.get("wide") else 0
    y["a_lo"] = kw + 8 if c.get("a_pair") else 0
    y["lda"] = y["a_off"] + y["a_lo"] + kw + 32
    y["off"] = 8 if c.get("wide") else 0
    y["o16_lo"] = y["Nout"] + 8 if c.get("o_pair") else 0
    y["w16"] = y["o16_lo"] + y["Nout"]
    y["ldo16"] = up8(y["off"] + y["w16"] + 24)
    y["ldo"] = up8(y["off"] + y["Nout"] + 24)                      # out32, aux16
    y["ldres"] = y["Nout"] + 16 if c.get("wide") else y["Nout"]
    y["ldrv"] = N + 8 if c.get("wide") else N
    y["batch"] = c.get("batch", 1)
    y["o_bstride"] = (y["M"] + 8) * y["ldo16"]
    y["w_bstride"] = (N + 8) * (9 * kw if c["form"] == "conv" else kw)
    return y


def gemm_args(c, **ptrs):
    """gdf_gemm_args of a case (pointers NULL, or 1 where only "set or not" matters, unless given): what both the dispatch test and the launch use"""
    y = layout(c)
    a = GemmArgs()
    p = lambda n, used: ctypes.c_void_p(ptrs.get(n, 1 if used else 0) or None)
    if c["form"] == "mx":
        a.mode, a.M, a.N, a.K, a.lda, a.mx = 0, c["M"], c["N"], c["K"], c["K"] + 32, 1
        return a
    if c["form"] == "conv_in":
        a.mode, a.B, a.H, a.Wd, a.Cin, a.N, a.stride = 1, c["B"], c["H"], c["W"], c["Cin"], c["N"], 1
        return a
    a.lda = y["lda"]
    if is_conv(c):
        a.mode, a.B, a.H, a.Wd, a.Cin = 1, c["B"], c["H"], c["W"], c["Cin"]
        a.stride, a.ups, a.pad0 = c.get("stride", 1), c.get("ups", 0), c.get("pad0", 0)
    else:
        a.mode, a.M, a.K = 0, c["M"], c["K"]
    a.N = c["N"]
    a.A, a.W = p("A", False), p("W", False)
    a.bias = p("bias", c.get("bias", True))
    a.rowvec = p("rowvec", c.get("rowvec"))
    a.rows_per_sample, a.ldrv = c.get("rowvec") or 0, y["ldrv"]
    a.res32, a.res16, a.ldres = p("res32", c.get("res") == "f32"), p("res16", c.get("res") == "f16"), y["ldres"]
    a.out16, a.ldo16 = p("out16", c.get("o16", True)), y["ldo16"]
    a.out32, a.ldo32 = p("out32", c.get("o32", True)), y["ldo"]
    a.aux16, a.ldaux = p("aux16", c.get("aux")), y["ldo"]
    a.geglu, a.bn, a.variant, a.no_superblock = int(bool(c.get("geglu"))), c.get("bn", 0), c.get("variant", 0), c.get("no_superblock", 0)
    a.splitk, a.splitk_ws = c.get("splitk", 0), p("splitk_ws", False)
    if y["batch"] > 1:
        a.batch, a.w_bstride, a.o_bstride = y["batch"], y["w_bstride"], y["o_bstride"]
    a.dit, a.act, a.rv_mul, a.rv_tok = c.get("dit", 0), c.get("act", 0), c.get("rv_mul", 0), c.get("rv_tok", 0)
    if c.get("rv_seg"):
        a.rv_seg_rows, a.rv_rps2 = c["rv_seg"]
    if c.get("qkn"):
        a.qkn_nq, a.qkn_eps = QKN["nq"], QKN["eps"]
        a.qkn_pos0, a.qkn_rps, a.qkn_seg_rows, a.qkn_pos1, a.qkn_rps2 = QKN["pos0"], QKN["rps"], QKN["seg_rows"], QKN["pos1"], QKN["rps2"]
        for n in ("qkn_wq", "qkn_wk", "rope_cos", "rope_sin"):
            setattr(a, n, p(n, False))
    a.bf16, a.out_f16 = c.get("bf16", 0), c.get("out_f16", 0)
    if c.get("scale"):
        a.acc_scale, a.out16_scale = 8.0, 0.125
    a.a_lo, a.o16_lo, a.cus = y["a_lo"], y["o16_lo"], c.get("cus", 0)
    return a


def kernel_name(L, a):
    n = L.gdf_op_gemm_kernel(ctypes.byref(a))
    return n.decode() if n is not None else None


# q heads [0, 128), k heads [128, 256), v columns from 256; two position bases: rows < 100 at 3 + r % 50, later rows at 60 + (r - 100) % 57
QKN = dict(nq=128, eps=1e-6, pos0=3, rps=50, seg_rows=100, pos1=60, rps2=57, npos=120)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, fp64 reference, emulation of the arithmetic contract
# ------------------------------------------------------------------------------------------------------------------------------
def e16(c):
    return torch.bfloat16 if c.get("bf16") else torch.float16


def make_inputs(c):
    y = layout(c)
    M, N, Nout, kw, dt = y["M"], y["N"], y["Nout"], y["Kw"], e16(c)
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    i = dict()
    a_off = float(c.get("a_off", 0.0))
    if is_conv(c):
        a = rn(c["B"], c["Cin"], c["H"], c["W"]) * (0.25 if a_off else 1.0) + a_off
        w = rn(y["batch"], N, c["Cin"], 3, 3) * (9 * kw) ** -0.5
    else:
        a = rn(M, kw) * (0.25 if a_off else 1.0) + a_off
        w = rn(y["batch"], N, kw) * kw ** -0.5
    if c.get("scale"):
        a = a.to(dt).float() * 0.125                               # stored x 2^-3 (exact), undone by acc_scale = 8
    if c.get("a_pair"):
        hi = a.to(dt)
        i["A"] = (hi, (a - hi.float()).to(dt))
    else:
        i["A"] = a.to(dt)
    i["W"] = w.to(dt)
    if c.get("bias", True):
        i["bias"] = rn(N) + float(c.get("bias_off", 0.0))
        if c.get("geglu"):
            i["bias"][N // 2:] += float(c.get("gate_off", 0.0)) - float(c.get("bias_off", 0.0))    # (h and the gate have their own offsets)
        if c.get("spikes"):                                        # a handful of results beyond the fp16 range, both signs
            i["bias"][5], i["bias"][N - 3] = 7.0e4, -9.0e4
    if c.get("rowvec"):
        rps = c["rowvec"]
        ns = rps if c.get("rv_tok") else (M + rps - 1) // rps + 8
        i["rowvec"] = rn(ns, N) + (1.0 if c.get("rv_mul") else 0.0)
    if c.get("res"):
        r = rn(M, Nout)
        i["res"] = r.half().float() if c["res"] == "f16" else r
    if c.get("qkn"):
        i["wq"], i["wk"] = 1.0 + 0.1 * rn(128), 1.0 + 0.1 * rn(128)
        ang = (rn(QKN["npos"], 64) * 3.0).repeat_interleave(2, dim=1)
        i["cos"], i["sin"] = torch.cos(ang), torch.sin(ang)
    return i


def value(x, dt):
    return x[0].to(dt) + x[1].to(dt) if isinstance(x, tuple) else x.to(dt)


def accumulate(c, i, b, dt):
    """A W^T of problem b in `dt` (fp64: the reference; fp32: the emulation) -> [M][N]"""
    A, W = value(i["A"], dt), i["W"][b].to(dt)
    if not is_conv(c):
        return A @ W.t()
    if c.get("ups"):
        A = F.interpolate(A, scale_factor=2.0, mode="nearest")
    s = c.get("stride", 1)
    if c.get("pad0"):
        # Downsample2D(padding = 0): F.pad (0, 1, 0, 1) + conv.  For an odd size the launch derives one more output row / column than that
        # reference has (OH = (H - 1) / stride + 1); those read one more row / column of zeros: F.pad (0, 2, 0, 2)
        o = F.conv2d(F.pad(A, (0, 1, 0, 1)), W, stride=s, padding=0)
        full = F.conv2d(F.pad(A, (0, 2, 0, 2)), W, stride=s, padding=0)
        assert torch.equal(full[:, :, :o.shape[2], :o.shape[3]], o)
        o = full
    else:
        o = F.conv2d(A, W, stride=s, padding=1)
    return o.permute(0, 2, 3, 1).reshape(-1, W.shape[0])


def sample_rows(c, M):
    r = torch.arange(M)
    rps = c["rowvec"]
    if c.get("rv_tok"):
        return r % rps
    s = r // rps
    if c.get("rv_seg"):
        seg, rps2 = c["rv_seg"]
        s = torch.where(r >= seg, (r - seg) // rps2, s)
    return s


def epilogue(c, i, acc):
    """the epilogue of kernels.h GemmParams in acc's dtype -> (v as stored to out32, pre-residual hook value or None)"""
    dt = acc.dtype
    M, N = acc.shape
    bias = i["bias"].to(dt) if "bias" in i else torch.zeros(N, dtype=dt)
    if c.get("geglu"):
        hg = acc + bias
        h, gt = hg[:, :N // 2], hg[:, N // 2:]
        return h * (0.5 * gt * (1.0 + torch.erf(gt * 2.0 ** -0.5))), None
    v = acc * (8.0 if c.get("scale") else 1.0) + bias
    if c.get("act"):
        v = 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    if c.get("qkn"):
        r = torch.arange(M)
        pos = torch.where(r >= QKN["seg_rows"], QKN["pos1"] + (r - QKN["seg_rows"]) % QKN["rps2"], QKN["pos0"] + r % QKN["rps"])
        cs, sn = i["cos"].to(dt)[pos], i["sin"].to(dt)[pos]
        v = v.clone()
        for h0, w in ((0, i["wq"]), (128, i["wk"])):
            x = v[:, h0:h0 + 128]
            t = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + QKN["eps"]) * w.to(dt)
            rot = torch.stack([-t[:, 1::2], t[:, 0::2]], -1).reshape(M, 128)
            v[:, h0:h0 + 128] = t * cs + rot * sn
    aux = None
    if c.get("aux") and c.get("dit") and c.get("rv_mul"):
        aux = v.clone()
    if c.get("rowvec"):
        rv = i["rowvec"].to(dt)[sample_rows(c, M)]
        v = v * rv if (c.get("dit") and c.get("rv_mul")) else v + rv
    if c.get("aux") and aux is None:
        aux = v.clone()
    if "res" in i:
        v = v + i["res"].to(dt)
    return v, aux


def store16(c, v, kind):
    """the value of a 16-bit store of fp32 `v` as fp64: kind 'out' (e16, out_f16: saturating fp16, pair: hi + lo) or 'aux' (fp16, MMDiT: saturating)"""
    v = v.float()
    if kind == "aux":
        return (v.clamp(-F16_MAX, F16_MAX) if c.get("dit") else v).half().double()
    if c.get("out_f16"):
        return v.clamp(-F16_MAX, F16_MAX).half().double()
    dt = e16(c)
    hi = v.to(dt)
    if c.get("o_pair"):
        return hi.double() + (v - hi.float()).to(dt).double()
    return hi.double()


def block_rel(got, ref):
    """worst relative L2 over the 16 x 16 blocks of an [M][N] result"""
    M, N = ref.shape
    pad = lambda x: F.pad(x, (0, -N % 16, 0, -M % 16)).reshape((M + 15) // 16, 16, (N + 15) // 16, 16)
    num, den = (pad(got - ref) ** 2).sum((1, 3)), (pad(ref) ** 2).sum((1, 3))
    return float((num / den).max().sqrt())


def tensor_rel(got, ref):
    return float((got - ref).norm() / ref.norm())


def bounds(c):
    bf = BF_FACTOR if (c.get("bf16") and not c.get("out_f16")) or c["form"] == "mx" else 1.0
    return dict(out16=(TOL_PAIR if c.get("o_pair") else TOL16) * bf, out32=TOL32, aux16=TOL16)


def reference(c, i):
    """per problem b: fp64 (out, aux) with the 16-bit saturation of the contract applied where the case asks for it, and the emulation's error"""
    y = layout(c)
    refs, emu = [], dict(out16=0.0, out32=0.0, aux16=0.0)
    osc = 0.125 if c.get("scale") else 1.0
    for b in range(y["batch"]):
        v64, a64 = epilogue(c, i, accumulate(c, i, b, torch.float64))
        v32, a32 = epilogue(c, i, accumulate(c, i, b, torch.float32))
        sat = lambda x: x.clamp(-F16_MAX, F16_MAX)
        r16 = sat(v64) if c.get("out_f16") else v64
        ra = sat(a64) if (a64 is not None and c.get("dit")) else a64
        refs.append(dict(out16=r16, out32=v64, aux16=ra))
        if c.get("o16", True):
            emu["out16"] = max(emu["out16"], block_rel(store16(c, v32 * osc, "out") / osc, r16))
        if c.get("o32", True):
            emu["out32"] = max(emu["out32"], block_rel(v32.double(), v64))
        if a64 is not None:
            emu["aux16"] = max(emu["aux16"], block_rel(store16(c, a32, "aux"), ra))
    return refs, emu


# ------------------------------------------------------------------------------------------------------------------------------
# launch into sentinel-filled outputs from poisoned operands
# ------------------------------------------------------------------------------------------------------------------------------
def off_ptr(t, elems):
    return t.data_ptr() + elems * t.element_size()


class Out:
    """a [batch][rows + 8][ld] output filled with the sentinel; the result is columns [off, off + width) of the first `rows` rows"""

    def __init__(self, batch, rows, ld, off, width, f32=False):
        self.batch, self.rows, self.ld, self.off, self.width, self.f32 = batch, rows, ld, off, width, f32
        self.buf = torch.full((batch, rows + 8, ld), SENT32 if f32 else SENT16, dtype=torch.int32 if f32 else torch.int16, device="cuda")
        self.ptr = off_ptr(self.buf, off)

    def read(self, gaps=()):
        """(result [batch][rows][width] raw, everything else still the sentinel); gaps: column ranges inside the result that must be sentinels"""
        raw = self.buf.cpu()
        mask = torch.zeros_like(raw, dtype=torch.bool)
        mask[:, :self.rows, self.off:self.off + self.width] = True
        for lo, hi in gaps:
            mask[:, :, self.off + lo:self.off + hi] = False
        intact = bool((raw[~mask] == (SENT32 if self.f32 else SENT16)).all())
        return raw[:, :self.rows, self.off:self.off + self.width].contiguous(), intact


def launch(L, c, i, **over):
    """one gdf_op_gemm_ex launch of case `c` (fields overridden by `over`) -> (rc, dict of fp64 results per problem, sentinels intact)"""
    c = dict(c, **over)
    y = layout(c)
    M, N, Nout, kw, dt = y["M"], y["N"], y["Nout"], y["Kw"], e16(c)
    keep = []                                                      # device tensors stay alive until the synchronize
    dev = lambda t: keep.append(t.cuda()) or keep[-1]
    ptrs = dict()
    # ---- A inside a poisoned allocation: lda > K, 8 more rows ----
    rowsA = c["B"] * c["H"] * c["W"] if is_conv(c) else M
    packed = c["form"] == "conv_in_ex"                             # pixels of 8 channels, the ones from Cin up zero (the format), poisoned rows after
    Ab = torch.full((rowsA + 8, 8 if packed else y["lda"]), POISON).to(dt)
    if packed:
        Ab[:rowsA] = 0
    parts = i["A"] if isinstance(i["A"], tuple) else (i["A"],)
    for n, part in enumerate(parts):
        m = part.permute(0, 2, 3, 1).reshape(rowsA, kw) if is_conv(c) else part
        c0 = y["a_off"] + n * y["a_lo"]
        Ab[:rowsA, c0:c0 + kw] = m
    Ad = dev(Ab)
    ptrs["A"] = off_ptr(Ad, y["a_off"])
    # ---- W: [batch][N + 8 rows][K], the extra rows poisoned ----
    kfull = 128 if packed else 9 * kw if c["form"] == "conv" else kw
    Wd = dev(torch.full((y["batch"], N + 8, kfull), POISON).to(dt))
    bias_d = None
    for b in range(y["batch"]):
        src = dev(i["W"][b].contiguous())
        dst = ctypes.c_void_p(off_ptr(Wd, b * y["w_bstride"]))
        if c["form"] == "conv":
            ok(L.gdf_op_relayout_conv3(P(src), dst, N, kw, stream()), L)
        elif packed:                                               # [N][16 taps][8 channels], taps from 9 up and channels from Cin up zero
            w8 = torch.zeros(N, 16, 8, dtype=dt)
            w8[:, :9, :kw] = i["W"][b].reshape(N, kw, 9).permute(0, 2, 1)
            Wd[b, :N] = dev(w8.reshape(N, 128))
        elif c.get("geglu"):
            bsrc, bias_d = dev(i["bias"]), dev(torch.zeros(N))
            ok(L.gdf_op_relayout_geglu(P(src), P(bsrc), dst, P(bias_d), N, kw, 16, stream()), L)
        else:
            Wd[b, :N] = src
    ptrs["W"] = Wd.data_ptr()
    if "bias" in i:
        ptrs["bias"] = (bias_d if bias_d is not None else dev(i["bias"])).data_ptr()
    if "rowvec" in i:
        rv = torch.full((i["rowvec"].shape[0], y["ldrv"]), POISON)
        rv[:, :N] = i["rowvec"]
        ptrs["rowvec"] = dev(rv).data_ptr()
    if "res" in i:
        r = torch.full((M, y["ldres"]), POISON)
        r[:, y["off"]:y["off"] + Nout] = i["res"]
        r = dev(r.half() if c["res"] == "f16" else r)
        ptrs["res16" if c["res"] == "f16" else "res32"] = off_ptr(r, y["off"])
    if c.get("qkn"):
        for n, k in (("qkn_wq", "wq"), ("qkn_wk", "wk"), ("rope_cos", "cos"), ("rope_sin", "sin")):
            ptrs[n] = dev(i[k].contiguous()).data_ptr()
    o16 = o32 = aux = None
    if c.get("o16", True):
        o16 = Out(y["batch"], M, y["ldo16"], y["off"], y["w16"])
        ptrs["out16"] = o16.ptr
    if c.get("o32", True):
        o32 = Out(1, M, y["ldo"], y["off"], Nout, f32=True)
        ptrs["out32"] = o32.ptr
    if c.get("aux"):
        aux = Out(1, M, y["ldo"], y["off"], Nout)
        ptrs["aux16"] = aux.ptr
    if c.get("splitk", 0) > 1:
        ptrs["splitk_ws"] = dev(torch.zeros(c["splitk"] * M * N)).data_ptr()
    a = gemm_args(c, **ptrs)
    rc = L.gdf_op_gemm_ex(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    res, intact = dict(), True
    if o16 is not None:
        raw, ok16 = o16.read(gaps=[(Nout, y["o16_lo"])] if y["o16_lo"] else ())
        intact &= ok16
        res["raw16"] = raw
        st = torch.float16 if c.get("out_f16") else dt
        hi = raw[:, :, :Nout].contiguous().view(st).double()
        res["out16"] = hi + raw[:, :, y["o16_lo"]:].contiguous().view(st).double() if y["o16_lo"] else hi
    if o32 is not None:
        raw, ok32 = o32.read()
        intact &= ok32
        res["raw32"] = raw
        res["out32"] = raw.view(torch.float32).double()
    if aux is not None:
        raw, oka = aux.read()
        intact &= oka
        res["rawaux"] = raw
        res["aux16"] = raw.view(torch.float16).double()
    return rc, res, intact


def check_outputs(c, res, refs, tag="GEMM_CASE"):
    bd, worst = bounds(c), dict()
    osc = 0.125 if c.get("scale") else 1.0
    for name in ("out16", "out32", "aux16"):
        if name not in res:
            continue
        for b, ref in enumerate(refs if name == "out16" else refs[:1]):
            got = res[name][b] / (osc if name == "out16" else 1.0)
            assert bool(torch.isfinite(got).all()), name
            t, blk = tensor_rel(got, ref[name]), block_rel(got, ref[name])
            worst[name] = max(worst.get(name, 0.0), blk)
            worst[name + "_tensor"] = max(worst.get(name + "_tensor", 0.0), t)
    print("%s %-44s %-44s " % (tag, c["id"], c["kernel"]) + " ".join("%s=%.2e" % kv for kv in sorted(worst.items()))
          + " bounds " + " ".join("%s=%.1e" % kv for kv in sorted(bd.items())))
    for name in ("out16", "out32", "aux16"):
        if name in worst:
            assert worst[name + "_tensor"] < bd[name] and worst[name] < bd[name], (name, worst, bd)
    return worst


def check_case(c, L=None, gpu=True):
    """the CPU half (branch, emulation headroom) and, with gpu=True, the launch and every assertion on its result"""
    L = L or lib()
    assert kernel_name(L, gemm_args(c)) == c["kernel"]                                   # 1. the instantiation the row claims
    if c["form"] in ("conv_in", "mx"):
        return check_own_entry(c, L, gpu)
    i = make_inputs(c)
    refs, emu = reference(c, i)
    bd = bounds(c)
    assert all(emu[n] <= bd[n] / 3 for n in emu), (emu, bd)                              # the inputs leave the bounds their headroom
    if not gpu:
        return emu
    rc, res, intact = launch(L, c, i)
    assert rc == 0, L.gdf_last_error().decode()
    assert intact, "written outside the result"                                           # 4.
    worst = check_outputs(c, res, refs)                                                   # 2., 3. (and 5.: poison would break them)
    if c.get("spikes"):                                                                   # beyond the fp16 range: +-65504, never inf
        assert float(res["out16"].max()) == F16_MAX and float(res["out16"].min()) == -F16_MAX
        assert float(res["aux16"].max()) == F16_MAX and float(res["aux16"].min()) == -F16_MAX
    if c.get("sb"):                                                                       # tile order must not change a bit
        rc2, res2, intact2 = launch(L, c, i, no_superblock=1)
        assert rc2 == 0 and intact2
        assert all(torch.equal(res[k], res2[k]) for k in res if k.startswith("raw"))
    if c.get("scale"):
        # the unscaled launch on the unscaled inputs: out32 equal, out16 equal times 2^-3, bit for bit (nothing near the fp16 subnormals)
        j = dict(i)
        j["A"] = (value(i["A"], torch.float32) * 8.0).to(e16(c))
        assert torch.equal(j["A"].float() * 0.125, i["A"].float()) and float(j["A"].float().abs().min()) >= 2.0 ** -10
        rc2, res2, intact2 = launch(L, c, j, scale=False)
        assert rc2 == 0 and intact2
        assert float(res2["out16"].abs().min()) * 0.125 >= 2.0 ** -14
        assert torch.equal(res["out16"], res2["out16"] * 0.125)
        if "out32" in res:
            assert torch.equal(res["out32"], res2["out32"])
    if c.get("splitk"):
        # a second launch: bit-identical (fixed summation order); the unsplit launch: within the fp32 bound (and the 16-bit bounds)
        rc2, res2, intact2 = launch(L, c, i)
        assert rc2 == 0 and intact2
        assert all(torch.equal(res[k], res2[k]) for k in res if k.startswith("raw"))
        rc3, res3, intact3 = launch(L, c, i, splitk=0)
        assert rc3 == 0 and intact3
        for name in ("out16", "out32", "aux16"):
            if name in res:
                assert block_rel(res[name][0], res3[name][0]) < (TOL32 if name == "out32" else bd[name]), name
    return worst


def check_own_entry(c, L, gpu):
    """conv_in (gdf_op_conv_in) and the fp8 GEMM (gdf_op_gemm_mx): same reference, bounds and sentinels through their own entry points"""
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    if c["form"] == "conv_in":
        B, H, W, Cin, N = c["B"], c["H"], c["W"], c["Cin"], c["N"]
        M = B * H * W
        x, w, bias = rn(B, Cin, H, W).half(), (rn(N, Cin, 3, 3) / 6.0).half(), rn(N)
        ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N)
        emu = F.conv2d(x.float(), w.float(), bias, padding=1).permute(0, 2, 3, 1).reshape(M, N).half().double()
        assert block_rel(emu, ref) <= TOL16 / 3
        if not gpu:
            return
        out = Out(1, M, N, 0, N)
        scratch = torch.zeros(M * 16 + N * 256, dtype=torch.uint8, device="cuda")
        xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
        ok(L.gdf_op_conv_in(P(xd), B, Cin, H, W, P(wd), P(bd), N, ctypes.c_void_p(out.ptr), P(scratch), stream()), L)
        torch.cuda.synchronize()
        raw, intact = out.read()
        assert intact, "written outside the result"
        check_outputs(c, dict(out16=raw.view(torch.float16).double()), [dict(out16=ref)])
        return
    M, N, K = c["M"], c["N"], c["K"]
    f8 = torch.float8_e4m3fn
    A8, W8 = rn(M, K).to(f8), (rn(N, K) * 0.5).to(f8)
    sa, sw = 2.0 ** torch.randint(-2, 3, (M,), generator=g).float(), 2.0 ** torch.randint(-3, 2, (N,), generator=g).float()
    bias, res = rn(N), rn(M, N)
    sw = sw * K ** -0.5                                            # (fold the 1 / sqrt(K) into the weight scale: any fp32 is allowed there)
    ref = (A8.double() @ W8.double().t()) * sa.double()[:, None] * sw.double()[None, :] + bias.double() + res.double()
    e32 = (A8.float() @ W8.float().t()) * (sa[:, None] * sw[None, :]) + bias + res
    assert block_rel(e32.bfloat16().double(), ref) <= TOL16 * BF_FACTOR / 3 and block_rel(e32.double(), ref) <= TOL32 / 3
    if not gpu:
        return
    lda = K + 32
    Ab = torch.full((M + 8, lda), 0x7E, dtype=torch.uint8)         # 0x7E = 448, the largest finite e4m3 value
    Ab[:M, :K] = A8.view(torch.uint8)
    Wb = torch.full((N + 8, K), 0x7E, dtype=torch.uint8)
    Wb[:N] = W8.view(torch.uint8)
    Ad, Wd, sad, swd, bd, rd = Ab.cuda(), Wb.cuda(), sa.cuda(), sw.cuda(), bias.cuda(), res.cuda()
    ld = up8(N + 24)
    o16, o32 = Out(1, M, ld, 0, N), Out(1, M, ld, 0, N, f32=True)
    ok(L.gdf_op_gemm_mx(P(Ad), lda, P(sad), P(Wd), P(swd), P(bd), 0, P(rd), N, ctypes.c_void_p(o16.ptr), ld, ctypes.c_void_p(o32.ptr), ld,
                        M, N, K, stream()), L)
    torch.cuda.synchronize()
    r16, i16 = o16.read()
    r32, i32 = o32.read()
    assert i16 and i32, "written outside the result"
    check_outputs(c, dict(out16=r16.view(torch.bfloat16).double(), out32=r32.view(torch.float32).double()), [dict(out16=ref, out32=ref)])


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_gemm_kernel(c):
    check_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,stride", [(128, 1), (932, 1), (826, 2)])
def test_conv_asymmetric_identity(variant, stride):
    """test_gemm_asymmetric_identity for a conv: a one-hot image (pixel p has channel p % 64 set) against weights that are a different number for
    every (output channel, input channel, tap), all exact in fp16: the fp32 output is the exact sum of at most nine weights, so a swapped tap,
    a transposed filter or a swapped MFMA row / column shows as a wrong number, not as noise"""
    L = lib()
    H, W, Cin, N = 7, 9, 64, 72
    x = torch.zeros(1, Cin, H, W)
    for p in range(H * W):
        x[0, (p * 5) % Cin, p // W, p % W] = 1.0
    o, ci, t = torch.meshgrid(torch.arange(N), torch.arange(Cin), torch.arange(9), indexing="ij")
    w = ((o * 37 + ci * 11 + t * 3) % 1021).float().reshape(N, Cin, 3, 3) / 8.0          # multiples of 1/8 below 128: exact in fp16
    c = conv("identity", None, 1, H, W, Cin, N, variant=variant, stride=stride, bias=False, o16=False)
    i = dict(A=x.half(), W=w.half()[None])
    ref = accumulate(c, i, 0, torch.float64)
    rc, res, intact = launch(L, c, i)
    assert rc == 0 and intact
    assert torch.equal(res["out32"][0], ref)


@pytest.mark.gpu
def test_rejected_arguments_launch_nothing():
    """arguments the query has no kernel for: an error from the launch, and no output element is written"""
    L = lib()
    for over in (dict(K=96), dict(bf16=1), dict(out_f16=1), dict(variant=826)):
        c = dict(dense("rejected", None, 200, 152, 64, variant=128), **over)
        assert kernel_name(L, gemm_args(c)) is None
        i = make_inputs(c)
        rc, res, intact = launch(L, c, i)
        assert rc != 0 and b"gemm_ex" in L.gdf_last_error()
        assert intact and bool((res["raw16"] == SENT16).all()) and bool((res["raw32"] == SENT32).all())
