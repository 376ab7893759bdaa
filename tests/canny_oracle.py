"""NumPy restatement of OpenCV 4.x cv::Canny(src8u, low, high, apertureSize=3, L2gradient=False) for 1- and 3-channel 8-bit images, the oracle of
the device Canny (csrc/canny.hip).  Written from the published algorithm; needs neither cv2 nor SciPy.

  classify(img, low, high) -> uint8 (H, W) class map, OpenCV's values: 2 strong, 0 candidate, 1 neither
  link(cls)                -> uint8 (H, W) 0 / 255: strong pixels and the candidates 8-connected to one through candidates / strong pixels
  canny(img, low, high)    -> link(classify(...))

Integer arithmetic throughout: 3x3 Sobel per channel on a REPLICATED pixel border, mag = |dx| + |dy|, the channel of the largest mag per pixel
(the first on a tie), a magnitude map whose border is ZERO, non-maximum suppression by the tan(22.5 deg) = 13573 / 2^15 test, two thresholds."""
import numpy as np
import torch
import torch.nn.functional as F

STRONG, CANDIDATE, NONE = 2, 0, 1


def sobel(img):
    """img uint8 (H, W) or (H, W, C) -> (mag, dx, dy) int32 (H, W) of the selected channel"""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.ndim == 3
    H, W, C = a.shape
    p = np.pad(a.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    mag = np.abs(gx) + np.abs(gy)
    m, dx, dy = mag[:, :, 0].copy(), gx[:, :, 0].copy(), gy[:, :, 0].copy()
    for c in range(1, C):
        take = mag[:, :, c] > m                      # strict: the first channel wins a tie
        m[take], dx[take], dy[take] = mag[:, :, c][take], gx[:, :, c][take], gy[:, :, c][take]
    return m, dx, dy


def classify(img, low=100, high=200):
    low, high = int(np.floor(low)), int(np.floor(high))
    if low > high:
        low, high = high, low
    m, dx, dy = sobel(img)
    H, W = m.shape
    mp = np.pad(m, 1)                                # the magnitude's border is zero
    at = lambda oy, ox: mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    tg22 = x * 13573
    tg67 = tg22 + (x << 16)
    horiz = y < tg22
    vert = ~horiz & (y > tg67)
    diag = ~horiz & ~vert
    keep_h = (m > at(0, -1)) & (m >= at(0, 1))
    keep_v = (m > at(-1, 0)) & (m >= at(1, 0))
    neg = (dx ^ dy) < 0                              # s = -1: compare (y - 1, x + 1) and (y + 1, x - 1)
    keep_d = np.where(neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    keep = (m > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    cls = np.full((H, W), NONE, np.uint8)
    cls[keep] = CANDIDATE
    cls[keep & (m > high)] = STRONG
    return cls


def link(cls):
    """queue flood from the strong pixels over 8-connected candidates"""
    cls = np.asarray(cls)
    H, W = cls.shape
    out = np.zeros((H, W), np.uint8)
    ys, xs = np.nonzero(cls == STRONG)
    out[ys, xs] = 255
    stack = list(zip(ys.tolist(), xs.tolist()))
    cand = (cls == CANDIDATE)
    while stack:
        y, x = stack.pop()
        for ny in range(max(y - 1, 0), min(y + 2, H)):
            for nx in range(max(x - 1, 0), min(x + 2, W)):
                if cand[ny, nx] and not out[ny, nx]:
                    out[ny, nx] = 255
                    stack.append((ny, nx))
    return out


def canny(img, low=100, high=200):
    return link(classify(img, low, high))


def quantise(x):
    """(..., ) float tensor in [-1, 1] -> uint8, as the reference's restore_from_tensor_to_image does it (VaeImageProcessor.postprocess):
    to fp32, (x / 2 + 0.5).clamp(0, 1) * 255, rounded half to even"""
    return ((x.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)


def smooth_noise(B, H, W, C=3, sigma=2.0, contrast=1.0, seed=0):
    """(B, H, W, C) uint8 (C = 0: (B, H, W)): Gaussian-smoothed normal noise per channel, stretched to `contrast` of 0 .. 255 around mid grey"""
    g = torch.Generator().manual_seed(seed)
    c = max(C, 1)
    r = int(4 * sigma + 0.5)
    k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float64) / sigma) ** 2)
    k = (k / k.sum())
    x = torch.randn(B * c, 1, H + 2 * r, W + 2 * r, generator=g, dtype=torch.float64)
    x = F.conv2d(F.conv2d(x, k.view(1, 1, -1, 1)), k.view(1, 1, 1, -1)).view(B, c, H, W)
    lo, hi = x.amin((2, 3), keepdim=True), x.amax((2, 3), keepdim=True)
    x = ((x - lo) / (hi - lo) - 0.5) * contrast + 0.5
    u = (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    return u[..., 0] if C == 0 else u


def steps():
    """the hand-checkable images of DESIGN.md 3.19: name -> (image uint8, expected edge mask bool)"""
    H, W = 12, 16
    out = {}
    v = np.zeros((H, W, 3), np.uint8); v[:, 6:] = 255
    e = np.zeros((H, W), bool); e[:, 5] = True
    out["vertical step, first bright column 6 -> column 5 on every row"] = (v, e)
    h = np.zeros((H, W, 3), np.uint8); h[4:] = 255
    e = np.zeros((H, W), bool); e[3] = True
    out["horizontal step, first bright row 4 -> row 3"] = (h, e)
    c0 = np.zeros((H, W, 3), np.uint8); c0[:, 0] = 255
    e = np.zeros((H, W), bool); e[:, 0] = True
    out["lone bright column 0 -> column 0"] = (c0, e)
    g40 = np.zeros((H, W, 3), np.uint8); g40[:, 6:, 1] = 40
    out["step of 40 in green only (mag 160): candidates only, empty output"] = (g40, np.zeros((H, W), bool))
    b60 = np.zeros((H, W, 3), np.uint8); b60[:, 6:, 2] = 60
    e = np.zeros((H, W), bool); e[:, 5] = True
    out["step of 60 in blue only (mag 240): strong"] = (b60, e)
    return out


def ties_image(H=48, W=80, seed=7):
    """(H, W, 3) uint8 whose channels 0 and 1 have the SAME magnitude at every pixel and different gradients: channel 0 = f(x) + h(y),
    channel 1 = f(x) + 127 - h(y), so dx agrees and dy has the opposite sign; in the diagonal case of the suppression the two channels compare
    different neighbours.  Which channel wins a tie decides the class of hundreds of pixels."""
    g = np.random.default_rng(seed)
    f = np.cumsum(g.integers(-30, 31, W)); f = (f - f.min()) * 127 // max(int(np.ptp(f)), 1)
    h = np.cumsum(g.integers(-30, 31, H)); h = (h - h.min()) * 127 // max(int(np.ptp(h)), 1)
    img = np.zeros((H, W, 3), np.uint8)
    img[..., 0] = (f[None, :] + h[:, None]).astype(np.uint8)
    img[..., 1] = (f[None, :] + 127 - h[:, None]).astype(np.uint8)
    return img


# ---- crafted class maps for the linking stage ----
def serpentine(H=96, W=160, strong=True):
    """a one-pixel-wide path of candidates over the whole map: every even row is full, rows 2k and 2k + 2 are joined by one pixel at the right end
    for even k and at the left end for odd k, so the path runs (0, 0) -> right -> down -> left -> down -> ...; the strong pixel (if any) is the path's
    LAST pixel"""
    cls = np.full((H, W), NONE, np.uint8)
    rows = (H + 1) // 2
    for k in range(rows):
        cls[2 * k, :] = CANDIDATE
        if k + 1 < rows:
            cls[2 * k + 1, W - 1 if k % 2 == 0 else 0] = CANDIDATE
    if strong:
        k = rows - 1                                           # row k is walked left -> right for even k
        cls[2 * k, W - 1 if k % 2 == 0 else 0] = STRONG
    return cls


def diagonal(H=96, W=160, tile=32):
    """two pure diagonal chains that step across tile CORNERS, each with its strong pixel at the far end: the main diagonal from (0, 0), through
    (tile - 1, tile - 1) -> (tile, tile) and so on, strong at its lower-right end; and an anti-diagonal through (tile - 1, 3 tile) -> (tile, 3 tile - 1),
    strong at its lower-left end"""
    assert W >= 3 * tile + 21 and H >= tile + 21
    cls = np.full((H, W), NONE, np.uint8)
    n = min(H, W)
    for i in range(n):
        cls[i, i] = CANDIDATE
    cls[n - 1, n - 1] = STRONG
    for j in range(-20, 21):
        cls[tile - 1 + j, 3 * tile - j] = CANDIDATE
    cls[tile - 1 + 20, 3 * tile - 20] = STRONG
    return cls


def random_map(H, W, p_cand, p_strong, seed):
    g = np.random.default_rng(seed)
    r = g.random((H, W))
    cls = np.full((H, W), NONE, np.uint8)
    cls[r < p_cand] = CANDIDATE
    cls[g.random((H, W)) < p_strong] = STRONG
    return cls


def link_stats(cls, edges):
    cand = cls == CANDIDATE
    return dict(strong=int((cls == STRONG).sum()), kept=int((cand & (edges > 0)).sum()), dropped=int((cand & (edges == 0)).sum()))
