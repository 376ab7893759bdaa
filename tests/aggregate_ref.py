"""Float64 reference and error bound of the bilinear aggregation (gdf_op_aggregate, components/postproc.py aggregate), shared by
tests/test_aggregate_cpu.py and tests/test_gpu_aggregate.py.

Coordinates are computed in numpy float32 with separately rounded operations, exactly as ATen's upsample_bilinear2d (align_corners = False)
defines them: scale = (float)in / out, src = max(0, scale * (dst + 0.5f) - 0.5f), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0,
l0 = 1 - l1.  The lambdas then go to float64 and the four taps are summed in float64.

Bound per element:  |got - ref| <= 1/2 ulp_out(ref) + (8 * 2^-24 + 4 u) M
  u        the fp32 ulp of max(src_y, src_x, 1)
  M        max |v| over source rows y0 - 1 .. y1 + 1 and columns x0 - 1 .. x1 + 1, clamped to the plane
  ulp_out  the fp16 ulp (subnormal range included) or the fp32 ulp of the reference
One rounding to the output type; fewer than 8 fp32 roundings in the blend; a compiler may or may not fuse scale * (dst + 0.5) - 0.5, which moves
each of the two coordinates by at most one ulp, hence each lambda by u and the value by at most 2 u * 2 M; the widened M covers a coordinate that
lands on the other side of an integer.  None of this is a measured figure."""
import ctypes as C

import numpy as np

f32 = np.float32


class AggSrc(C.Structure):
    """gdf_agg_src of include/gdf_ops.h (same field order)"""
    _fields_ = [("ptr", C.c_void_p), ("f32", C.c_int), ("sb", C.c_long), ("sc", C.c_long), ("sy", C.c_long), ("sx", C.c_long),
                ("C", C.c_int), ("H", C.c_int), ("W", C.c_int), ("coff", C.c_int)]


# (the table goes as a plain address: an AggSrc array converts to it, whichever module set the argtypes of the shared handle last)
AGG_ARGTYPES = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]


def bind(L):
    L.gdf_op_aggregate.restype, L.gdf_op_aggregate.argtypes = C.c_int, AGG_ARGTYPES
    L.gdf_last_error.restype = C.c_char_p
    L.gdf_abi_version.restype = C.c_int
    return L


def coords(out, inn):
    """-> (src fp32, i0, i1, l0 float64, l1 float64) of every destination index"""
    scale = f32(inn) / f32(out)
    d = np.arange(out, dtype=f32)
    s = np.maximum(f32(0), (scale * (d + f32(0.5))).astype(f32) - f32(0.5)).astype(f32)
    i0 = s.astype(np.int32)
    i1 = i0 + (i0 < inn - 1)
    l1 = (s - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return s, i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def _window_max(a, lo, hi, axis):
    """max of `a` over index windows [lo[k], hi[k]] (each at most 4 long) along `axis` -> that axis gets len(lo) entries"""
    out = None
    for k in range(4):
        t = np.take(a, np.minimum(lo + k, hi), axis=axis)
        out = t if out is None else np.maximum(out, t)
    return out


def reference(v, OH, OW, out_f32=False):
    """v: (B, C, H, W) array (fp16 / fp32 values) -> (ref float64 (B, C, OH, OW), bound float64 of the same shape)"""
    v = np.asarray(v, dtype=np.float64)
    H, W = v.shape[2:]
    sy, y0, y1, ly0, ly1 = coords(OH, H)
    sx, x0, x1, lx0, lx1 = coords(OW, W)
    top, bot = v[:, :, y0, :], v[:, :, y1, :]
    ly0, ly1 = ly0[None, None, :, None], ly1[None, None, :, None]
    ref = ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])
    a = np.abs(v)
    M = _window_max(a, np.maximum(y0 - 1, 0), np.minimum(y1 + 1, H - 1), 2)
    M = _window_max(M, np.maximum(x0 - 1, 0), np.minimum(x1 + 1, W - 1), 3)
    u = np.spacing(np.maximum(np.maximum(sy[:, None], sx[None, :]), f32(1)).astype(f32)).astype(np.float64)
    if out_f32:
        ulp = np.spacing(np.abs(ref).astype(f32)).astype(np.float64)
    else:
        e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -24)))
        ulp = 2.0 ** (np.maximum(e, -14.0) - 10.0)
    return ref, 0.5 * ulp + (8.0 * 2.0 ** -24 + 4.0 * u[None, None]) * M


def check(got, v, OH, OW, out_f32=False, what=""):
    """assert the bound for got (B, C, OH, OW) against the reference of v; prints the worst share of the bound first"""
    ref, bound = reference(v, OH, OW, out_f32)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    share = float((err / bound).max())
    print("aggregate %s %s -> %dx%d %s: worst element at %.3f of the bound" % (what, tuple(np.shape(v)), OH, OW, "fp32" if out_f32 else "fp16", share))
    assert np.isfinite(err).all() and share <= 1.0, (what, share)
    return share
