"""NumPy restatement of Pillow's 8-bit bicubic resize (ImagingResample, whole-image box) as DESIGN.md 3.22 states it: the specification of
csrc/preproc.hip.  Python floats are IEEE doubles and nothing here fuses a multiply with an add, so every value below is the one the C code
computes; int() truncates like C's cast.  CASES is the shape list the CPU and GPU tests share."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# source (h, w) -> S
CASES = [((90, 70), 64), ((70, 90), 64), ((33, 47), 128), ((300, 200), 64), ((64, 64), 64), ((64, 100), 64), ((100, 64), 64),
         ((517, 389), 128), ((1, 1), 16), ((2, 3), 16), ((1000, 30), 32), ((255, 257), 256)]
KINDS = ("rgb", "rgb01", "l")


def axis_pairs():
    """every (in, out) pair of CASES whose axis is resampled, plus 2048 -> 64 (ksize 129, the largest the C ABI takes)"""
    pairs = []
    for (h, w), s in CASES:
        for n in (w, h):
            if n != s and (n, s) not in pairs:
                pairs.append((n, s))
    return pairs + [(2048, 64)]


def source(kind, h, w, seed=0):
    g = np.random.default_rng([seed, h, w, KINDS.index(kind)])
    if kind == "rgb":
        return g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "rgb01":                                          # bytes 0 / 255 only: bicubic overshoots on both sides, both clamps work
        return (g.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return g.integers(0, 256, (h, w), dtype=np.uint8)


def bicubic(x):
    x = abs(x)
    if x < 1.0:
        return ((1.5 * x - 2.5) * x) * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def ksize_of(n_in, n_out):
    fs = max(n_in / n_out, 1.0)
    return int(math.ceil(2.0 * fs)) * 2 + 1


def coeffs(n_in, n_out):
    """-> bounds int32 (n_out, 2) = (xmin, xmax), kk int32 (n_out, ksize), ksize"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        for x, v in enumerate(k):
            kk[xx, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pass(src, n_out):
    """one pass along axis 0 of an integer array (n_in, ...) -> uint8 (n_out, ...)"""
    bounds, kk, _ = coeffs(src.shape[0], n_out)
    s = src.astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, xmax = bounds[xx]
        w = kk[xx, :xmax].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (s[xmin:xmin + xmax] * w).sum(0)
        assert np.abs(acc).max() < 2 ** 31                       # the C code accumulates in int
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(a, out_h, out_w):
    """uint8 (h, w) or (h, w, 3) -> Image.fromarray(a).resize((out_w, out_h)) as an array: horizontal pass first, then vertical; a pass whose
    axis already has the target size is skipped"""
    h, w = a.shape[:2]
    if w != out_w:
        a = np.swapaxes(_pass(np.swapaxes(a, 0, 1), out_w), 0, 1)
    if h != out_h:
        a = _pass(a, out_h)
    return np.ascontiguousarray(a)


def resize_rgb(a, size):
    """np.array(Image.fromarray(a).resize((size, size)).convert("RGB"))"""
    r = resize_u8(a, size, size)
    return np.ascontiguousarray(np.repeat(r[..., None], 3, 2) if r.ndim == 2 else r)


def normalise(u8_hwc3):
    """the (3, S, S) fp32 row image_processor.preprocess makes of those bytes: (fp32(u) / 255) * 2 - 1"""
    x = u8_hwc3.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray((x * np.float32(2.0) - np.float32(1.0)).transpose(2, 0, 1))
