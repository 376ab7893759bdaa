"""Float64 oracle, seeded generator and acceptance rules of the pixel-classifier ensemble (gdf_pixcls_*, components/postproc.py
PixelClassifierEnsemble / predict_labels), shared by tests/test_pixel_classifier_cpu.py and tests/test_gpu_pixel_classifier.py.

The op (reference scarce_segmentation/segmentation/pixel_classifier.py): M networks Linear ReLU BatchNorm1d Linear ReLU BatchNorm1d Linear
(eval mode: running statistics, eps 1e-5) on every pixel; per model the argmax (lowest index) and the entropy of its softmax; the mean softmax,
renormalised, and its entropy -sum p log(clamp(p, eps32, 1 - eps32)); js = H(mean) - mean_m H_m; the label = the most frequent per-model label,
the smallest among equally frequent ones (torch.mode's rule).

Oracle: the UNFOLDED network in float64 from the inputs as given (an fp16 map is exact in float64).

Bounds: no fixed constant.  They come from the reference's own arithmetic at run time, the same layers evaluated by torch in fp32 on the CPU:
  logit bound   8 x the worst relative L2 error, per (model, block of 16 consecutive pixels), of those fp32 logits against the oracle.  The factor 8
                is the project's margin for a different fp32 summation order (tests/test_gpu_dit_rows.py).
  js bound      8 x the worst |js32 - js64| of the reference's Categorical chain run in fp32 and in fp64 on the same (fp32) logits.
  ambiguity     the relative L2 bound of a block limits every single logit error in it by tol = bound x ||oracle block||_2; a pixel is ambiguous when
                any model's oracle top-2 gap is <= 2 tol.  Off ambiguous pixels the labels must equal the oracle's; at most 5 % of a case may be
                ambiguous (a condition on the inputs: the check cannot pass vacuously).
Generator (seeded; correlated enough to give O(1) logit gaps): Linear weights 1.5 N(0, 1) / sqrt(fan_in), biases 0.3 N; BatchNorm gamma 1 + 0.2 N,
beta 0.2 N, mean 0.4 + 0.1 N, var 0.3 + 0.2 U; every parameter fp32.  Features randn times a per-channel scale in [0.25, 4]."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from aggregate_ref import AggSrc

BLOCK, MARGIN, BN_EPS = 16, 8.0, 1e-5
EPS32 = float(torch.finfo(torch.float32).eps)
GDF_ERR_ARG, GDF_ERR_UNSUPPORTED = 1, 4
vp, ci = C.c_void_p, C.c_int


def bind(L):
    L.gdf_pixcls_create.restype, L.gdf_pixcls_create.argtypes = ci, [ci] * 5 + [vp] * 6 + [C.POINTER(vp)]
    L.gdf_pixcls_destroy.restype, L.gdf_pixcls_destroy.argtypes = None, [vp]
    L.gdf_pixcls_workspace.restype, L.gdf_pixcls_workspace.argtypes = C.c_size_t, [vp, ci, ci, ci]
    L.gdf_pixcls_predict.restype, L.gdf_pixcls_predict.argtypes = ci, [vp, vp, ci, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.gdf_last_error.restype = C.c_char_p
    return L


def agg_src(ptr, f32, strides, shape):
    s = AggSrc()
    s.ptr, s.f32 = ptr, int(f32)
    s.sb, s.sc, s.sy, s.sx = strides
    _, s.C, s.H, s.W = shape
    return s


def widths(K):
    """the reference's two architectures"""
    return (128, 32) if K < 30 else (256, 128)


def gen_models(C_, M, K, seed, prefix=""):
    """M state dicts of the reference's pixel_classifier(K, C_) (keys layers.{0,2,3,5,6}.*, optionally behind `prefix`), fp32"""
    g = torch.Generator().manual_seed(seed)
    h1, h2 = widths(K)
    out = []
    for _ in range(M):
        sd = {}
        for name, (o, i) in (("0", (h1, C_)), ("3", (h2, h1)), ("6", (K, h2))):
            sd[name + ".weight"] = 1.5 * torch.randn(o, i, generator=g) / i ** 0.5
            sd[name + ".bias"] = 0.3 * torch.randn(o, generator=g)
        for name, n in (("2", h1), ("5", h2)):
            sd[name + ".weight"] = 1 + 0.2 * torch.randn(n, generator=g)
            sd[name + ".bias"] = 0.2 * torch.randn(n, generator=g)
            sd[name + ".running_mean"] = 0.4 + 0.1 * torch.randn(n, generator=g)
            sd[name + ".running_var"] = 0.3 + 0.2 * torch.rand(n, generator=g)
            sd[name + ".num_batches_tracked"] = torch.tensor(100)
        out.append({prefix + "layers." + k: v.float() for k, v in sd.items()})
    return out


def gen_features(B, C_, H, W, f32, seed):
    """(B, C_, H, W) contiguous, fp16 or fp32: randn times a per-channel scale in [0.25, 4] (log-uniform)"""
    g = torch.Generator().manual_seed(seed)
    scale = 0.25 * 16.0 ** torch.rand(C_, generator=g)
    v = torch.randn(B, C_, H, W, generator=g) * scale[None, :, None, None]
    return v if f32 else v.half()


def rows(v):
    """logical (B, C, H, W) map -> (P, C), pixel p = (b H + y) W + x"""
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1])


def _strip(sd):
    out = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        out[k[len("layers."):]] = v
    return out


def network(sd, x, dtype):
    """the unfolded network of one state dict on rows x (P, C) in `dtype` -> logits (P, K)"""
    p = {k: v.to(dtype) for k, v in _strip(sd).items() if v.is_floating_point()}
    h = x.to(dtype)
    for lin, bn in (("0", "2"), ("3", "5")):
        h = F.relu(F.linear(h, p[lin + ".weight"], p[lin + ".bias"]))
        h = (h - p[bn + ".running_mean"]) / torch.sqrt(p[bn + ".running_var"] + BN_EPS) * p[bn + ".weight"] + p[bn + ".bias"]
    return F.linear(h, p["6.weight"], p["6.bias"])


def sequential(sd):
    """the reference's nn.Sequential of one state dict, eval mode, fp32 on the CPU"""
    p = _strip(sd)
    h1, c = p["0.weight"].shape
    h2, k = p["3.weight"].shape[0], p["6.weight"].shape[0]
    net = torch.nn.Sequential(torch.nn.Linear(c, h1), torch.nn.ReLU(), torch.nn.BatchNorm1d(h1), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                              torch.nn.BatchNorm1d(h2), torch.nn.Linear(h2, k))
    net.load_state_dict(p)
    return net.eval()


class Module(torch.nn.Module):
    """stand-in of the reference's pixel_classifier module: the same `layers` Sequential and state-dict keys"""

    def __init__(self, sd):
        super().__init__()
        self.layers = sequential(sd)
        self.eval()

    def forward(self, x):
        return self.layers(x)


def oracle_logits(sds, v):
    """-> (M, P, K) float64"""
    x = rows(v).double()
    return torch.stack([network(sd, x, torch.float64) for sd in sds])


def reference_logits(sds, v):
    """the reference's arithmetic: nn.Sequential in fp32 on the CPU -> (M, P, K) fp32"""
    x = rows(v).float()
    with torch.no_grad():
        return torch.stack([sequential(sd)(x) for sd in sds])


def block_norms(t):
    """(M, P, K) -> (M, ceil(P / BLOCK)) L2 norms over blocks of BLOCK consecutive pixels"""
    M, P, K = t.shape
    nb = (P + BLOCK - 1) // BLOCK
    pad = torch.zeros(M, nb * BLOCK, K, dtype=torch.float64)
    pad[:, :P] = t.double()
    return pad.reshape(M, nb, BLOCK * K).norm(dim=2)


def block_rel(got, want):
    """-> (M, blocks) relative L2 error of got against want (float64 oracle)"""
    return block_norms(got.double() - want) / block_norms(want)


def js_chain(logits, dtype):
    """the reference's Categorical chain (pixel_classifier.py:79-102) on logits (M, P, K) in `dtype` -> js (P,)"""
    lg = logits.to(dtype)
    ent, mean = [], None
    for m in range(lg.shape[0]):
        ent.append(Categorical(logits=lg[m]).entropy())
        sm = torch.softmax(lg[m], 1)
        mean = sm if mean is None else mean + sm
    mean = mean / lg.shape[0]
    return Categorical(mean).entropy() - torch.mean(torch.stack(ent), 0)


def js_formula(logits):
    """the float64 formula of the op on logits (M, P, K): the mean's entropy with the fp32-epsilon clamp -> (P,) float64"""
    ls = torch.log_softmax(logits.double(), 2)
    p = ls.exp()
    ent = -(p * ls).sum(2).mean(0)
    mean = p.mean(0)
    mean = mean / mean.sum(1, keepdim=True)
    return -(mean * torch.log(mean.clamp(EPS32, 1 - EPS32))).sum(1) - ent


def lowest_argmax(logits):
    """(M, P, K) -> (M, P) int64, the lowest index among equal maxima"""
    a = logits.numpy()
    return torch.from_numpy((a == a.max(2, keepdims=True)).argmax(2))


def smallest_mode(labels, K):
    """(M, P) -> (P,) the most frequent label, the smallest among equally frequent ones"""
    counts = torch.stack([(labels == c).sum(0) for c in range(K)], 1)            # (P, K)
    a = counts.numpy()
    return torch.from_numpy((a == a.max(1, keepdims=True)).argmax(1))


def top_k(js_row):
    """the reference's expression, including its P < 10 quirk"""
    return js_row.sort()[0][-int(js_row.shape[0] / 10):].mean()


class Bounds:
    """the bounds of one case, taken from the reference's fp32 arithmetic on that case's inputs"""

    def __init__(self, sds, v):
        self.oracle = oracle_logits(sds, v)
        ref = reference_logits(sds, v)
        self.K = self.oracle.shape[2]
        self.ref_rel = float(block_rel(ref, self.oracle).max())
        self.logit = MARGIN * self.ref_rel
        self.ref_js = float((js_chain(ref, torch.float32).double() - js_chain(ref, torch.float64)).abs().max())
        self.js = MARGIN * self.ref_js
        self.tol = self.logit * block_norms(self.oracle)                         # (M, blocks): the absolute error a logit of that block may have
        top2 = self.oracle.topk(2, dim=2)[0] if self.K > 1 else None
        P = self.oracle.shape[1]
        tol_p = self.tol.repeat_interleave(BLOCK, dim=1)[:, :P]
        self.ambiguous = ((top2[..., 0] - top2[..., 1]) <= 2 * tol_p).any(0) if top2 is not None else torch.zeros(P, dtype=torch.bool)
        self.labels = smallest_mode(lowest_argmax(self.oracle), self.K)
        self.reference = ref

    def check_logits(self, got, what=""):
        rel = block_rel(got, self.oracle)
        print("pixel classifier %s: worst block error %.3e, bound %.3e (reference fp32: %.3e)" % (what, float(rel.max()), self.logit, self.ref_rel))
        assert bool(torch.isfinite(rel).all()) and float(rel.max()) <= self.logit, (what, float(rel.max()), self.logit)

    def check_labels(self, got, what=""):
        got = torch.as_tensor(got).reshape(-1).long()
        P = got.shape[0]
        clear = ~self.ambiguous
        wrong = int((got[clear] != self.labels[clear]).sum())
        print("pixel classifier %s: %d pixels, %d ambiguous, %d wrong off them" % (what, P, int(self.ambiguous.sum()), wrong))
        assert int(self.ambiguous.sum()) <= 0.05 * P, (what, "more than 5 % of the pixels are ambiguous", int(self.ambiguous.sum()), P)
        assert wrong == 0, (what, wrong)
