"""Kernel-level parity of every attention kernel the dispatcher can pick (-m gpu), through gdf_op_attention_ex.

CASES is the map from kernel instantiation to the test that runs it; tests/test_attention_dispatch_cpu.py asserts (without a
GPU) that every instantiation a shipped model or a sweep of legal arguments reaches has a row here.  To add a case for a new
instantiation: add a row whose arguments make the dispatcher choose it and write the symbol into `kernel`.

Every case draws its inputs with a fixed seed, rounds them to the element type, computes softmax attention of the rounded
values in fp64 on the CPU per (sample, head), and asserts
  1. gdf_op_attention_kernel(args) == the `kernel` of the row (a case that falls into another branch fails),
  2. whole-tensor relative L2: output 2e-3, maps 1e-3 (bf16 output: x 8, three fewer mantissa bits),
  3. the same bounds per query row (D outputs / one query's probabilities), which a whole-tensor norm cannot see,
  4. nothing is written outside the result (sentinel columns, rows and map tail intact).
Before it looks at the GPU result a case asserts that an emulation of the kernels' arithmetic contract (fp64 scores,
probabilities rounded to 16 bit before P V, unrounded row sum, 16-bit output) stays under bound / 3 per output row, and under
the fp16 rounding limit 2^-11 per map row (MAP_ROUNDING below): the inputs, not the bounds, are what gets changed if that fails.
"""
import ctypes
import zlib

import pytest
import torch

from ops_binding import AttnArgs, lib, stream

TOL_O, TOL_MAP, BF_FACTOR = 2e-3, 1e-3, 8.0
SENTINEL = 0x5A5A            # fp16 205.25, bf16 1.5e16: finite in either type
# A map row is one rounding of the exact probabilities to fp16: every normal element is within 2^-11 relative, so the row's relative L2 is
# too (measured on the rows of this table: 2.9e-4 at Sk = 520 to 4.1e-4 at Sk = 77; short rows average over fewer roundings).  That is the
# headroom the emulation is held to for maps: a third of the 1e-3 bound is below what rounding alone gives a 77-key row, whatever the input.
MAP_ROUNDING = 2.0 ** -11
MASKED_FILL = 1e4            # K / V rows at and beyond kv_len[b]: large, finite; the kernel must ignore them


def AK(D, QW=1, NW=4, BF=False, OCC=2, PV16=False, QKP=False):
    t = lambda v: "true" if v else "false"
    return "attn_kernel<%d, %d, %d, %s, %d, %s, %s>" % (D, QW, NW, t(BF), OCC, t(PV16), t(QKP))


def MK(D, FULL, OCC=2, LW=False, BF=False):
    t = lambda v: "true" if v else "false"
    return "attn_map_kernel<%d, %s, %d, %s, %s>" % (D, t(FULL), OCC, t(LW), t(BF))


def case(id, kernel, B, heads, Sq, Sk, D, **kw):
    return dict(id=id, kernel=kernel, B=B, heads=heads, Sq=Sq, Sk=Sk, D=D, **kw)


# per-sample key counts of the kv_len cases (Sk = 300: whole tail tiles are masked): 1, around a tile edge, Sk - 1, Sk, > Sk (clamped)
KVL = [1, 63, 64, 65, 299, 300, 305]

CASES = [
    # ---- 64 query rows per wave (QW = 2): B * heads * ceil(Sq / 128) > 512 workgroups ----
    case("d64-qw2-ragged", AK(64, 2), 5, 16, 1000, 1000, 64),                  # ragged last 256-row block and ragged last key tile
    case("d64-qw2-even", AK(64, 2), 5, 16, 1024, 320, 64),                     # Sq a multiple of 256
    case("d32-qw2-ragged", AK(32, 2), 5, 16, 1000, 200, 32),
    case("d40-qw2-pv16-ragged", AK(40, 2, PV16=True), 5, 16, 1000, 1000, 40),
    case("d40-qw2-pv16-cross", AK(40, 2, PV16=True), 10, 16, 512, 77, 40),
    case("d64-qw2-peaked", AK(64, 2), 5, 16, 1000, 1000, 64, gain=4, spike=True),
    case("d40-qw2-pv16-peaked", AK(40, 2, PV16=True), 5, 16, 1000, 1000, 40, gain=4, spike=True),
    # ---- D = 128: 8 waves (Sq >= 1024) and 4 waves, fp16 and bf16, plain and joint ----
    case("d128-8w-f16", AK(128, 1, 8), 1, 2, 1100, 1100, 128),
    case("d128-8w-bf16", AK(128, 1, 8, BF=True), 1, 2, 1100, 1100, 128, bf16=1),
    case("d128-8w-f16-joint", AK(128, 1, 8), 2, 1, 1112, 1112, 128, seg_T=72),
    case("d128-8w-bf16-joint", AK(128, 1, 8, BF=True), 2, 1, 1112, 1112, 128, seg_T=72, bf16=1),
    case("d128-8w-f16-peaked", AK(128, 1, 8), 1, 2, 1100, 1100, 128, gain=4, spike=True),
    case("d128-8w-bf16-peaked", AK(128, 1, 8, BF=True), 1, 2, 1100, 1100, 128, bf16=1, gain=4, spike=True),
    case("d128-4w-f16", AK(128), 2, 2, 300, 77, 128),
    case("d128-4w-bf16", AK(128, BF=True), 2, 2, 300, 300, 128, bf16=1),
    case("d128-4w-f16-joint", AK(128), 2, 2, 140, 140, 128, seg_T=40),
    case("d128-4w-bf16-joint", AK(128, BF=True), 2, 2, 140, 140, 128, seg_T=40, bf16=1),
    # ---- D = 72 (PixArt): PV16 kernel and its map kernels ----
    case("d72-cross", AK(72, PV16=True), 2, 2, 300, 77, 72),
    case("d72-self", AK(72, PV16=True), 1, 3, 520, 520, 72),
    case("d72-cross-kvlen", AK(72, PV16=True), 3, 2, 300, 77, 72, kv_len=[1, 40, 77]),
    case("d72-self-peaked", AK(72, PV16=True), 1, 3, 520, 520, 72, gain=4, spike=True),
    case("d72-cross-map", MK(72, False), 2, 2, 300, 77, 72, map=True),
    case("d72-cross-map-kvlen", MK(72, False), 3, 2, 300, 77, 72, map=True, kv_len=[1, 40, 77]),
    case("d72-self-map", MK(72, False), 1, 2, 520, 520, 72, map=True),
    # ---- kv_len (prefix key mask), map and no map ----
    case("d40-kvlen", AK(40, PV16=True), 7, 2, 130, 300, 40, kv_len=KVL),
    case("d64-kvlen", AK(64), 7, 2, 130, 300, 64, kv_len=KVL),
    case("d72-kvlen", AK(72, PV16=True), 7, 2, 130, 300, 72, kv_len=KVL),
    case("d128-kvlen", AK(128), 7, 2, 130, 300, 128, kv_len=KVL),
    case("d40-kvlen-map", MK(40, False), 7, 2, 130, 300, 40, kv_len=KVL, map=True),
    case("d64-kvlen-map", MK(64, False), 7, 2, 128, 320, 64, kv_len=KVL, map=True),      # a FULL shape: the mask takes it off the FULL kernel
    case("d72-kvlen-map", MK(72, False), 7, 2, 130, 300, 72, kv_len=KVL, map=True),
    case("d128-kvlen-map", MK(128, False), 7, 2, 130, 300, 128, kv_len=KVL, map=True),
    # ---- one K / V set shared by all samples (kv_bstride = 0): bit-identical to the per-sample launch on repeated K / V ----
    case("d40-shared-kv-77", AK(40, PV16=True), 4, 2, 200, 77, 40, shared_kv=True),
    case("d40-shared-kv-128", AK(40, PV16=True), 4, 2, 200, 128, 40, shared_kv=True),
    case("d64-shared-kv-77", AK(64), 4, 2, 200, 77, 64, shared_kv=True),
    case("d64-shared-kv-128", AK(64), 4, 2, 200, 128, 64, shared_kv=True),
    case("d64-shared-kv-map", MK(64, True), 4, 2, 128, 128, 64, shared_kv=True, map=True),
    # ---- MMDiT joint sequence with `self-map` / `cross-map` ----
    case("d128-joint-maps-f16", MK(128, False), 2, 2, 320, 320, 128, seg_T=64, map=True, map2=True),
    case("d128-joint-maps-bf16", MK(128, False, BF=True), 2, 2, 320, 320, 128, seg_T=64, map=True, map2=True, bf16=1),
    case("d128-joint-maps-f16-ragged", MK(128, False), 1, 3, 140, 140, 128, seg_T=40, map=True, map2=True),
    case("d128-joint-maps-bf16-ragged", MK(128, False, BF=True), 1, 3, 140, 140, 128, seg_T=40, map=True, map2=True, bf16=1),
    case("d128-joint-crossmap-only", MK(128, False), 1, 2, 140, 140, 128, seg_T=40, map2=True),
    # ---- o_scale: the stored output is the unscaled one times 2^-3, bit for bit (v offset: no output near the fp16 subnormals) ----
    case("d64-oscale", AK(64), 2, 2, 200, 77, 64, o_scale=0.125, v_offset=3.0),
    case("d128-joint-oscale", AK(128), 2, 2, 140, 140, 128, seg_T=40, o_scale=0.125, v_offset=3.0),
    # ---- o as a bf16 (hi, lo) pair from fp16 internals ----
    case("d128-joint-pair-bf16", AK(128), 2, 2, 140, 140, 128, seg_T=40, pair_out=True),
    # ---- q / k / v as split fp16 pairs (40 <= D <= 80) ----
    case("d40-qkv-pairs", AK(40, 1, 8, OCC=1, QKP=True), 2, 2, 300, 300, 40, qkv_pair=True),
    case("d64-qkv-pairs", AK(64, 1, 8, OCC=1, QKP=True), 2, 2, 300, 77, 64, qkv_pair=True),
    case("d72-qkv-pairs", AK(72, 1, 4, OCC=1, QKP=True), 2, 2, 300, 77, 72, qkv_pair=True),
    case("d80-qkv-pairs", AK(80, 1, 4, OCC=1, QKP=True), 2, 2, 130, 200, 80, qkv_pair=True),
    # ---- the remaining 32-rows-per-wave kernels ----
    case("d32-4w", AK(32), 2, 2, 100, 100, 32),
    case("d40-4w-pv16", AK(40, PV16=True), 1, 8, 1024, 77, 40),
    case("d64-4w", AK(64), 1, 2, 1000, 300, 64),
    case("d80-pv16", AK(80, PV16=True), 2, 2, 300, 300, 80),
    case("d80-pv16-peaked", AK(80, PV16=True), 2, 2, 300, 300, 80, gain=4, spike=True),
    case("d160", AK(160), 2, 2, 100, 300, 160),
    # ---- every attn_map_kernel form ----
    case("d32-map-full-lw", MK(32, True, 3, True), 1, 2, 128, 128, 32, map=True),
    case("d40-map-full-lw", MK(40, True, 3, True), 2, 2, 256, 384, 40, map=True),
    case("d32-map-full", MK(32, True, 3), 1, 2, 128, 192, 32, map=True),
    case("d40-map-full", MK(40, True, 3), 1, 2, 256, 64, 40, map=True),
    case("d64-map-full", MK(64, True), 1, 2, 128, 192, 64, map=True),
    case("d72-map-full", MK(72, True), 1, 2, 256, 192, 72, map=True),
    case("d80-map-full", MK(80, True), 1, 2, 128, 192, 80, map=True),
    case("d128-map-full", MK(128, True), 1, 2, 128, 192, 128, map=True),
    case("d160-map-full", MK(160, True), 1, 2, 128, 64, 160, map=True),
    case("d32-map-ragged", MK(32, False), 2, 2, 130, 100, 32, map=True),
    case("d40-map-ragged", MK(40, False), 2, 2, 130, 100, 40, map=True),
    case("d64-map-ragged", MK(64, False), 2, 2, 128, 100, 64, map=True),          # ragged keys only
    case("d80-map-ragged", MK(80, False), 2, 2, 130, 128, 80, map=True),          # ragged queries only
    case("d128-map-ragged", MK(128, False), 2, 2, 130, 100, 128, map=True),
    case("d160-map-ragged", MK(160, False), 2, 2, 130, 100, 160, map=True),
    case("d128-map-bf16", MK(128, False, BF=True), 2, 2, 128, 192, 128, map=True, bf16=1),
]


def attn_args(c, **ptrs):
    """gdf_attn_args of a case (pointers NULL unless given): what both the dispatch test and the launch use"""
    C = c["heads"] * c["D"]
    a = AttnArgs()
    wq = 2 * C if c.get("qkv_pair") else C
    wo = 2 * C if c.get("pair_out") else C
    a.ldq = a.ldk = a.ldv = wq
    a.ldo = wo + 8
    a.B, a.heads, a.Sq, a.Sk, a.D = c["B"], c["heads"], c["Sq"], c["Sk"], c["D"]
    a.kv_bstride = 0 if c.get("shared_kv") else c["Sk"]
    a.scale = 0.0
    a.seg_T = c.get("seg_T", 0)
    a.bf16 = c.get("bf16", 0)
    a.o_lo = C if c.get("pair_out") else 0
    a.o_pair_bf16 = 1 if c.get("pair_out") else 0
    a.q_lo = a.kv_lo = C if c.get("qkv_pair") else 0
    a.o_scale = c.get("o_scale", 0.0)
    # only whether these are set matters to the dispatcher
    a.map = ctypes.c_void_p(ptrs.get("map", 1 if c.get("map") else 0) or None)
    a.map2 = ctypes.c_void_p(ptrs.get("map2", 1 if c.get("map2") else 0) or None)
    a.kv_len = ctypes.c_void_p(ptrs.get("kv_len", 1 if c.get("kv_len") else 0) or None)
    for n in ("q", "k", "v", "o"):
        setattr(a, n, ctypes.c_void_p(ptrs.get(n) or None))
    return a


def kernel_name(L, a):
    n = L.gdf_op_attention_kernel(ctypes.byref(a))
    return n.decode() if n is not None else None


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, fp64 reference, emulation of the arithmetic contract
# ------------------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """q (B, Sq, C), k / v (Bk, Sk, C) as tensors of the element type; for split pairs a (hi, lo) tuple of fp16 tensors"""
    B, heads, Sq, Sk, D = c["B"], c["heads"], c["Sq"], c["Sk"], c["D"]
    C = heads * D
    dt = torch.bfloat16 if c.get("bf16") else torch.float16
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    Bk = 1 if c.get("shared_kv") else B
    q = torch.randn(B, Sq, C, generator=g) * float(c.get("gain", 1))
    k = torch.randn(Bk, Sk, C, generator=g)
    v = torch.randn(Bk, Sk, C, generator=g) + float(c.get("v_offset", 0.0))
    if c.get("spike"):                                       # one key per sample is a (gained) query: one-hot rows, a late rescale
        k[:, (3 * Sk) // 4] = q[:Bk, 7]
    if c.get("kv_len"):
        for b, n in enumerate(c["kv_len"]):
            n = max(1, min(n, Sk))
            k[b, n:] = MASKED_FILL
            v[b, n:] = MASKED_FILL
    if c.get("qkv_pair"):
        split = lambda x: (x.half(), (x - x.half().float()).half())
        return split(q), split(k), split(v)
    return q.to(dt), k.to(dt), v.to(dt)


def value64(x):
    return x[0].double() + x[1].double() if isinstance(x, tuple) else x.double()


def row_rel(got, ref):
    """worst relative L2 over rows (last dim)"""
    return float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max())


def tensor_rel(got, ref):
    return float((got - ref).norm() / ref.norm())


def reference(c, q, k, v, want_probs):
    """fp64 softmax attention of the rounded inputs per (sample, head) -> ref o (B, Sq, C), probabilities (B, heads, Sq, Sk) or
    None, and the worst per-row error of the emulated kernel arithmetic (output, map)."""
    B, heads, Sq, Sk, D = c["B"], c["heads"], c["Sq"], c["Sk"], c["D"]
    dt = torch.bfloat16 if c.get("bf16") else torch.float16
    q64, k64, v64 = value64(q), value64(k), value64(v)
    ref = torch.empty(B, Sq, heads * D, dtype=torch.float64)
    probs = torch.empty(B, heads, Sq, Sk, dtype=torch.float64) if want_probs else None
    emu_o = emu_m = 0.0
    for b in range(B):
        bk = 0 if c.get("shared_kv") else b
        n = max(1, min(c["kv_len"][b], Sk)) if c.get("kv_len") else Sk
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            s = (q64[b, :, sl] @ k64[bk, :n, sl].t()) * D ** -0.5
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            l = e.sum(-1, keepdim=True)
            p = e / l
            o = p @ v64[bk, :n, sl]
            ref[b, :, sl] = o
            emu = ((e.to(dt).double() @ v64[bk, :n, sl]) / l).to(dt).double()
            emu_o = max(emu_o, row_rel(emu, o))
            if want_probs:
                probs[b, h].zero_()
                probs[b, h, :, :n] = p
                emu_m = max(emu_m, row_rel(p.half().double(), p))
    return ref, probs, emu_o, emu_m


def to_rows(x, T):
    """(B, S, W) -> the activation matrix rows: sample-major, or region-major [B x T text][B x (S - T) image] for T > 0"""
    W = x.shape[-1]
    if T == 0:
        return x.reshape(-1, W).contiguous()
    return torch.cat([x[:, :T].reshape(-1, W), x[:, T:].reshape(-1, W)], 0).contiguous()


def from_rows(r, B, S, T):
    W = r.shape[-1]
    if T == 0:
        return r.reshape(B, S, W)
    return torch.cat([r[:B * T].reshape(B, T, W), r[B * T:].reshape(B, S - T, W)], 1)


def device_rows(x, T):
    """device matrix of an input: (rows, C), or (rows, 2C) = [hi | lo] for a split pair"""
    if isinstance(x, tuple):
        return torch.cat([to_rows(x[0], T), to_rows(x[1], T)], 1).contiguous().cuda()
    return to_rows(x, T).cuda()


def launch(L, c, q, k, v, **over):
    """one gdf_op_attention_ex launch of case `c` (fields overridden by `over`) into sentinel-filled buffers that are sized exactly
    for the arguments.  Returns (rc, o (B, Sq, Wo) on the CPU, map, map2, sentinels_intact)."""
    c = dict(c, **over)
    B, heads, Sq, Sk, D, T = c["B"], c["heads"], c["Sq"], c["Sk"], c["D"], c.get("seg_T", 0)
    C = heads * D
    dt = torch.bfloat16 if c.get("bf16") else torch.float16
    qd, kd, vd = device_rows(q, T), device_rows(k, T), device_rows(v, T)
    wo = 2 * C if c.get("pair_out") else C
    rows, ldo = B * Sq, wo + 8
    assert qd.shape == (rows, 2 * C if c.get("qkv_pair") else C)
    assert kd.shape[0] == (1 if c.get("shared_kv") else B) * Sk and kd.shape == vd.shape
    obuf = torch.full(((rows + 8) * ldo,), SENTINEL, dtype=torch.int16, device="cuda")
    ptrs = dict(q=qd.data_ptr(), k=kd.data_ptr(), v=vd.data_ptr(), o=obuf.data_ptr())
    Si = Sq - T
    mbuf = m2buf = kvl = None
    n_map = B * heads * (Si * Si if T else Sq * Sk)
    n_map2 = B * heads * Si * T
    if c.get("map"):
        mbuf = torch.full((n_map + Sk,), SENTINEL, dtype=torch.int16, device="cuda")
        ptrs["map"] = mbuf.data_ptr()
    if c.get("map2"):
        m2buf = torch.full((n_map2 + Sk,), SENTINEL, dtype=torch.int16, device="cuda")
        ptrs["map2"] = m2buf.data_ptr()
    if c.get("kv_len"):
        kvl = torch.tensor(c["kv_len"], dtype=torch.int32, device="cuda")
        assert kvl.numel() == B
        ptrs["kv_len"] = kvl.data_ptr()
    a = attn_args(c, **ptrs)
    rc = L.gdf_op_attention_ex(ctypes.byref(a), stream())
    torch.cuda.synchronize()
    o2 = obuf.cpu().view(rows + 8, ldo)
    intact = bool((o2[rows:] == SENTINEL).all()) and bool((o2[:, wo:] == SENTINEL).all())
    o = from_rows(o2[:rows, :wo].contiguous().view(dt), B, Sq, T)
    mp = mp2 = None
    if mbuf is not None:
        m = mbuf.cpu()
        intact = intact and bool((m[n_map:] == SENTINEL).all())
        mp = m[:n_map].view(torch.float16).view(B, heads, Si, Si) if T else m[:n_map].view(torch.float16).view(B, heads, Sq, Sk)
    if m2buf is not None:
        m = m2buf.cpu()
        intact = intact and bool((m[n_map2:] == SENTINEL).all())
        mp2 = m[:n_map2].view(torch.float16).view(B, heads, Si, T)
    untouched = bool((o2 == SENTINEL).all()) and all(bool((m.cpu() == SENTINEL).all()) for m in (mbuf, m2buf) if m is not None)
    return rc, o, mp, mp2, intact, untouched


def check_case(c, L=None, gpu=True):
    """the CPU half (branch, emulation headroom) and, with gpu=True, the launch and every assertion on its result"""
    L = L or lib()
    B, heads, Sq, Sk, D, T = c["B"], c["heads"], c["Sq"], c["Sk"], c["D"], c.get("seg_T", 0)
    C = heads * D
    assert kernel_name(L, attn_args(c)) == c["kernel"]                                  # 1. the branch the row claims
    tol_o = TOL_O * (BF_FACTOR if c.get("bf16") else 1.0)
    want_maps = bool(c.get("map") or c.get("map2"))
    q, k, v = make_inputs(c)
    ref, probs, emu_o, emu_m = reference(c, q, k, v, want_maps)
    assert emu_o <= tol_o / 3 and emu_m <= MAP_ROUNDING, (emu_o, emu_m)                 # the inputs leave the bounds their headroom
    if not gpu:
        return dict(emu_o=emu_o, emu_m=emu_m)
    rc, o, mp, mp2, intact, _ = launch(L, c, q, k, v)
    assert rc == 0, L.gdf_last_error().decode()
    assert intact, "written outside the result"                                          # 4.
    sc = c.get("o_scale", 0.0) or 1.0
    rowsD = lambda x: x.reshape(B, Sq, heads, D)
    if c.get("pair_out"):
        hi, lo = o[..., :C].contiguous().view(torch.bfloat16).double(), o[..., C:].contiguous().view(torch.bfloat16).double()
        got = hi + lo
    else:
        got = o.double() / sc
    assert bool(torch.isfinite(got).all())
    res = dict(o_tensor=tensor_rel(got, ref), o_row=row_rel(rowsD(got), rowsD(ref)), emu_o=emu_o, emu_m=emu_m)
    if want_maps:
        want = [(mp, probs[:, :, T:, T:] if T else probs, "map"), (mp2, probs[:, :, T:, :T] if T else None, "map2")]
        for gotm, refm, name in want:
            if gotm is None:
                continue
            gm = gotm.double()
            assert bool(torch.isfinite(gm).all())
            res[name + "_tensor"], res[name + "_row"] = tensor_rel(gm, refm), row_rel(gm, refm)
            if c.get("kv_len"):                                                          # masked keys: a full row, probability exactly 0
                for b, n in enumerate(c["kv_len"]):
                    assert float(gm[b, :, :, max(1, min(n, Sk)):].abs().max() if n < Sk else 0.0) == 0.0
    print("ATTN_CASE %-28s %-48s " % (c["id"], c["kernel"]) + " ".join("%s=%.2e" % kv for kv in sorted(res.items()))
          + " bound_o=%.1e bound_map=%.1e" % (tol_o, TOL_MAP))
    assert res["o_tensor"] < tol_o and res["o_row"] < tol_o, res                         # 2. and 3.
    for name in ("map", "map2"):
        if name + "_tensor" in res:
            assert res[name + "_tensor"] < TOL_MAP and res[name + "_row"] < TOL_MAP, res

    if c.get("shared_kv"):        # the per-sample launch on the repeated K / V set: bit for bit
        rep = lambda x: x.expand(B, -1, -1).contiguous()
        rc2, o2, mp_2, _, intact2, _ = launch(L, c, q, rep(k), rep(v), shared_kv=False)
        assert rc2 == 0 and intact2
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16))
        if mp is not None:
            assert torch.equal(mp.view(torch.int16), mp_2.view(torch.int16))
    if c.get("o_scale"):          # the unscaled launch times the power of two: bit for bit (exact in fp16 away from the subnormals)
        rc2, o2, _, _, intact2, _ = launch(L, c, q, k, v, o_scale=0.0)
        assert rc2 == 0 and intact2
        assert float(o2.float().abs().min()) * sc >= 2.0 ** -14
        assert torch.equal(o.float(), o2.float() * sc)
    if c.get("pair_out"):
        # hi is the bf16 rounding of the fp32 result the plain launch rounds to fp16.  bf16(fp16(x)) and bf16(x) differ where fp16(x)
        # sits on a bf16 tie (about 1 element in 16), so: within half a bf16 ulp + half an fp16 ulp (2^-25 in the fp16 subnormals) everywhere,
        # equal for most
        rc2, o2, _, _, intact2, _ = launch(L, c, q, k, v, pair_out=False)
        assert rc2 == 0 and intact2
        plain = o2.double()
        assert bool(((hi - plain).abs() <= plain.abs() * (2.0 ** -8 + 2.0 ** -11) + 2.0 ** -25).all())
        assert float((hi == plain.to(torch.bfloat16).double()).double().mean()) > 0.85
        res_hi = row_rel(rowsD(hi), rowsD(ref))
        print("ATTN_CASE %-28s hi alone: tensor=%.2e row=%.2e" % (c["id"], tensor_rel(hi, ref), res_hi))
        assert tensor_rel(got, ref) < tensor_rel(hi, ref) and res["o_row"] < res_hi
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_attention_kernel(c):
    check_case(c)


@pytest.mark.gpu
def test_joint_maps_reject_text_length_not_multiple_of_8():
    """seg_T = 12 with a map: an 8-key chunk would straddle the text / image boundary -> an error, no name, nothing written"""
    L = lib()
    c = case("d128-joint-maps-seg12", None, 1, 2, 140, 140, 128, seg_T=12, map=True, map2=True)
    assert kernel_name(L, attn_args(c)) is None
    q, k, v = make_inputs(c)
    rc, _, _, _, _, untouched = launch(L, c, q, k, v)
    assert rc != 0 and b"attention_ex" in L.gdf_last_error()
    assert untouched
    c2 = dict(c, map=False, map2=False)                         # without maps the same sequence is served
    assert kernel_name(L, attn_args(c2)) == AK(128)
