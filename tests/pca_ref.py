"""Oracle, fp32 restatement, input generators and bounds for the PCA op (csrc/pca.hip, include/gdf_ops.h gdf_op_pca / gdf_op_pca_rgb).

What the reference computes (feature_visualization.py:84-101, plot_pca) for one map f (C, H, W) taken as n = H W samples of C features:
sklearn PCA(n_components=3).fit(f).transform(f): the per-channel mean is subtracted, the samples are projected onto the three leading eigenvectors
of the sample covariance (divisor n - 1), each signed so that its entry of largest magnitude is positive (svd_flip(u_based_decision=False)); then
(p - min) / (max - min) per component, (. * 255).astype(uint8) and a nearest resize of the short side to 512 (Pillow's rule: source index
floor((dst + 0.5) in / out), clamped).

  oracle(x, ...)      all of it in float64 (numpy eigh of the centred covariance)
  restate32(x, ...)   the same pipeline in float32 throughout: the arithmetic a float32 implementation of the reference would have
  Bounds              MARGIN (the project's 8, tests/pixel_classifier_ref.py) x the restatement's own worst error against the oracle ON THE SAME
                      INPUT, for components, projection and the normalised picture; eigenvalues likewise, relative to lambda_1.  uint8: within 1
                      of the oracle everywhere, equal wherever the oracle's float64 n * 255 is farther than 255 x the picture bound from an integer
No figure in this file was measured on the code under test."""
import ctypes as C
import functools

import numpy as np

from aggregate_ref import AggSrc
from pixel_classifier_ref import MARGIN

GDF_ERR_ARG, GDF_ERR_UNSUPPORTED = 1, 4
TOL, MAX_ITER = 2.0 ** -20, 256
vp, ci = C.c_void_p, C.c_int
WS_ARGTYPES = [ci] * 6
PCA_ARGTYPES = [vp, ci, ci, ci, ci, C.c_float, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
RGB_ARGTYPES = [vp, ci, ci, ci, ci, vp, ci, ci, vp]


def bind(L):
    L.gdf_op_pca_workspace.restype, L.gdf_op_pca_workspace.argtypes = C.c_size_t, WS_ARGTYPES
    L.gdf_op_pca.restype, L.gdf_op_pca.argtypes = ci, PCA_ARGTYPES
    L.gdf_op_pca_rgb.restype, L.gdf_op_pca_rgb.argtypes = ci, RGB_ARGTYPES
    L.gdf_last_error.restype = C.c_char_p
    L.gdf_abi_version.restype = ci
    return L


def agg_src(ptr, f32, strides, shape):
    s = AggSrc()
    s.ptr, s.f32 = ptr, int(f32)
    s.sb, s.sc, s.sy, s.sx = strides
    _, s.C, s.H, s.W = shape
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# generators: fp16 values with a chosen population spectrum through a random orthogonal basis
# ------------------------------------------------------------------------------------------------------------------------------
def spectrum(kind, C_):
    i = np.arange(C_, dtype=np.float64)
    if kind in ("planted", "bigmean"):
        s = np.full(C_, 0.03)
        s[:3] = (1.0, 0.5, 0.25)[:min(3, C_)]
    elif kind == "slow":
        s = 0.55 * 0.97 ** (i - 3)
        s[:3] = (1.0, 0.8, 0.6)[:min(3, C_)]
    elif kind == "geometric":
        s = 0.9 ** i
    else:
        raise ValueError(kind)
    return s


def features(kind, B, C_, H, W, seed, f32=False):
    """-> (B, C_, H, W) numpy array, fp16 (or fp32: the fp16 values plus fp32 noise of 1e-4) : every image B H W independent normal samples with the
    population covariance Q diag(spectrum) Q^T; `bigmean` adds channel means 8 x N(0, 1) (eight times the largest spread)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((C_, C_)))
    z = rng.standard_normal((B * H * W, C_)) * np.sqrt(spectrum(kind, C_))
    x = z @ q.T
    if kind == "bigmean":
        x = x + 8.0 * rng.standard_normal(C_)
    x = x.reshape(B, H, W, C_).transpose(0, 3, 1, 2).astype(np.float16)
    if f32:
        x = x.astype(np.float32) + (1e-4 * rng.standard_normal(x.shape)).astype(np.float32)
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------------------------------------------------------------------
# the pipeline in one precision
# ------------------------------------------------------------------------------------------------------------------------------
def out_size(H, W, size):
    """the short side goes to `size`, the long side to int(size * long / short) (torchvision's Resize(int)); None keeps the grid"""
    if size is None:
        return H, W
    if H <= W:
        return int(size), int(size * W / H)
    return int(size * H / W), int(size)


def nearest_index(n_out, n_in):
    """Pillow's nearest rule, in integers: floor((dst + 0.5) n_in / n_out), clamped"""
    d = np.arange(n_out, dtype=np.int64)
    return np.minimum((2 * d + 1) * n_in // (2 * n_out), n_in - 1)


def sign_rule(v):
    """rows of v signed so that the entry of largest magnitude (the first among equals) is positive"""
    idx = np.argmax(np.abs(v), axis=1)
    s = np.sign(v[np.arange(v.shape[0]), idx])
    s[s == 0] = 1
    return v * s[:, None]


def _pipeline(x, k, joint, size, dt, gram=False):
    """x (B, C, H, W) -> dict of arrays in dtype dt.  gram: the covariance as (X^T X - n mu mu^T) / (n - 1) (what the op must NOT do)"""
    B, C_, H, W = x.shape
    xs = x.astype(dt).transpose(0, 2, 3, 1).reshape(B, H * W, C_)
    groups = [xs.reshape(1, B * H * W, C_)[0]] if joint else [xs[b] for b in range(B)]
    mean, comp, var, tot, proj = [], [], [], [], []
    for X in groups:
        n = X.shape[0]
        mu = X.mean(axis=0, dtype=dt)
        Xc = X - mu
        if gram:
            cov = (X.T @ X - dt(n) * np.outer(mu, mu)) / dt(n - 1)
        else:
            cov = (Xc.T @ Xc) / dt(n - 1)
        w, v = np.linalg.eigh(cov)
        order = np.argsort(-w, kind="stable")[:k]
        V = sign_rule(v[:, order].T.astype(dt))
        mean.append(mu); comp.append(V); var.append(w[order].astype(dt)); tot.append(np.trace(cov, dtype=dt)); proj.append((Xc @ V.T).astype(dt))
    G = len(groups)
    proj = np.stack(proj).reshape(B, H * W, k) if not joint else proj[0].reshape(B, H * W, k)
    proj = proj.transpose(0, 2, 1).reshape(B, k, H, W)
    out = dict(mean=np.stack(mean), components=np.stack(comp), variance=np.stack(var), total_variance=np.array(tot, dtype=dt), projection=proj, G=G)
    if k >= 3:
        out.update(colour(proj[:, :3], joint, size, dt))
    return out


def colour(proj, joint, size, dt=np.float64):
    """projection (B, 3, H, W) -> picture n (B, H, W, 3) in [0, 1], n255 = n * 255, u8 (B, OH, OW, 3) after the nearest resize.  A component of zero
    range gives 0."""
    proj = proj.astype(dt)
    B, _, H, W = proj.shape
    ax = (0, 2, 3) if joint else (2, 3)
    lo, hi = proj.min(axis=ax, keepdims=True), proj.max(axis=ax, keepdims=True)
    rng = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(rng > 0, (proj - lo) / rng, dt(0)).astype(dt)
    n255 = (n * dt(255)).astype(dt)
    OH, OW = out_size(H, W, size)
    iy, ix = nearest_index(OH, H), nearest_index(OW, W)
    pick = lambda a: a[:, :, iy][:, :, :, ix].transpose(0, 2, 3, 1)  # noqa: E731
    return dict(picture=n.transpose(0, 2, 3, 1), n255=pick(n255), u8=pick(n255.astype(np.uint8)))


def oracle(x, k=3, joint=False, size=None):
    return _pipeline(np.asarray(x), k, joint, size, np.float64)


def restate32(x, k=3, joint=False, size=None, gram=False):
    return _pipeline(np.asarray(x), k, joint, size, np.float32, gram=gram)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------
def errors(got, want):
    """worst absolute errors of a result dict against the oracle's: components, projection, picture; eigenvalues relative to lambda_1"""
    e = dict(components=float(np.abs(got["components"].astype(np.float64) - want["components"]).max()),
             projection=float(np.abs(got["projection"].astype(np.float64) - want["projection"]).max()),
             variance=float((np.abs(got["variance"].astype(np.float64) - want["variance"]) / want["variance"][:, :1]).max()))
    if "picture" in got and "picture" in want:
        e["picture"] = float(np.abs(got["picture"].astype(np.float64) - want["picture"]).max())
    return e


class Bounds:
    def __init__(self, x, k=3, joint=False, size=None):
        self.want = oracle(x, k, joint, size)
        self.ref = restate32(x, k, joint, size)
        self.ref_err = errors(self.ref, self.want)
        self.bound = {key: MARGIN * v for key, v in self.ref_err.items()}

    def excluded(self):
        """bool array over the oracle's uint8 values: n * 255 within 255 x the picture bound of an integer (a value there may differ by 1).  The
        extremes themselves are not excluded: 0 / range and range / range are exact in any precision."""
        n255 = self.want["n255"]
        return (np.abs(n255 - np.round(n255)) <= 255.0 * self.bound["picture"]) & (n255 != 0.0) & (n255 != 255.0)

    def check_u8(self, u8, what=""):
        want = self.want["u8"]
        assert u8.shape == want.shape and u8.dtype == np.uint8, (u8.shape, want.shape)
        diff = np.abs(u8.astype(np.int32) - want.astype(np.int32))
        ex = self.excluded()
        print("pca %s: uint8 differing %d of %d, %d in the excluded zone (%.3f %%)" % (what, int((diff > 0).sum()), diff.size, int(ex.sum()),
                                                                                   100.0 * ex.mean()))
        assert int(diff.max()) <= 1, "a uint8 value is more than 1 from the oracle"
        assert not bool((diff[~ex] != 0).any()), "a uint8 value outside the excluded zone differs from the oracle"

    def check(self, got, what=""):
        """got: dict with mean, components, variance, total_variance, projection (numpy), optionally picture"""
        err = errors(got, self.want)
        for key, v in err.items():
            print("pca %s: %s error %.3e, bound %.3e (fp32 restatement: %.3e)" % (what, key, v, self.bound[key], self.ref_err[key]))
        for key, v in err.items():
            assert np.isfinite(v) and v <= self.bound[key], (what, key, v, self.bound[key])
        # the mean and the trace: MARGIN x the restatement's error as well, with the rounding of one fp32 value as the floor
        for key in ("mean", "total_variance"):
            w = self.want[key]
            e = float(np.abs(got[key].astype(np.float64) - w).max())
            b = MARGIN * max(float(np.abs(self.ref[key].astype(np.float64) - w).max()), 2.0 ** -24 * float(np.abs(w).max()))
            print("pca %s: %s error %.3e, bound %.3e" % (what, key, e, b))
            assert e <= b, (what, key, e, b)


# name -> (kind, B, C, H, W, seed, f32, layout, joint, size)
CASES = {
    "C 3 on 6 x 6, k = C": ("planted", 1, 3, 6, 6, 1, False, "nchw", False, None),
    "C 20 on 5 x 7": ("planted", 1, 20, 5, 7, 2, False, "nchw", False, None),
    "C 77 on 16 x 16 NCHW": ("planted", 1, 77, 16, 16, 3, False, "nchw", False, 512),
    "C 96 on 24 x 24 channels-last": ("planted", 1, 96, 24, 24, 4, False, "cl", False, None),
    "C 320 on 32 x 32 fp32": ("planted", 1, 320, 32, 32, 5, True, "nchw", False, None),
    "C 1280 on 16 x 16": ("planted", 1, 1280, 16, 16, 6, False, "cl", False, None),
    "8 x 20 to size 64": ("planted", 1, 40, 8, 20, 7, False, "nchw", False, 64),
    "big mean": ("bigmean", 1, 64, 16, 16, 8, False, "nchw", False, None),
    "slow": ("slow", 1, 64, 24, 24, 9, False, "nchw", False, None),
    "geometric": ("geometric", 1, 64, 24, 24, 10, False, "cl", False, None),
    "joint B 2": ("planted", 2, 48, 12, 12, 11, False, "nchw", True, None),
    "independent B 2": ("planted", 2, 48, 12, 12, 12, False, "cl", False, None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x numpy (B, C, H, W), layout, joint, size, Bounds); computed once per process and shared"""
    kind, B, C_, H, W, seed, f32, layout, joint, size = CASES[name]
    x = features(kind, B, C_, H, W, seed, f32)
    return x, layout, joint, size, Bounds(x, 3, joint, size)
