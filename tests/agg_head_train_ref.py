"""Float64 oracle, seeded generators, acceptance rule, emulation and ctypes binding of the trainable aggregation head (gdf_agghead_wgrad,
gdf_agghead_update, gdf_agghead_create_device, components/postproc.py TrainableAggregationHead), shared by tests/test_agg_head_train_cpu.py and
tests/test_gpu_agg_head_train.py.

The op (reference correspondence/task-corres.py train(): loss.backward() through aggregation_network.out): the weight gradient of
nn.Conv2d(Cin, Cout, 3, padding=1, bias=False), dW[co, ci, dy, dx] = sum_{b, y, x} G[b, co, y, x] X[b, ci, y + dy - 1, x + dx - 1].

Oracle: the weight gradient of F.conv2d in float64 from the inputs as given.
Reference arithmetic: the same in fp32 on the CPU, what the reference's backward computes.
Bound: no fixed constant.  The error is the relative L2 error per input channel (its 9 taps over all Cout) against the oracle; a result passes
when its worst channel is within MARGIN = 8 x the worst channel of the reference arithmetic on the same inputs: the rule and the margin of
pixel_classifier_ref.Bounds and agg_head_ref.Bounds.
Generators (seeded): features as pixel_classifier_ref.gen_features; G = randn x 1e-5; heavy-tailed G = randn x 2^(-30 u) x 1e-4 with u uniform
per element."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

from agg_head_ref import Network, agg_src, gen_features, gen_weight  # noqa: F401
from pixel_classifier_ref import MARGIN

GDF_ERR_ARG = 1
vp, ci = C.c_void_p, C.c_int
PW, PH, ROWS, CT = 32, 4, 128, 32                                            # the kernel's pixel patch, and a workgroup's output / input channels


def bind(L):
    L.gdf_agghead_create.restype, L.gdf_agghead_create.argtypes = ci, [ci, ci, vp, vp, C.POINTER(vp)]
    L.gdf_agghead_create_device.restype, L.gdf_agghead_create_device.argtypes = ci, [ci, ci, vp, vp, vp, C.POINTER(vp)]
    L.gdf_agghead_update.restype, L.gdf_agghead_update.argtypes = ci, [vp, vp, vp]
    L.gdf_agghead_destroy.restype, L.gdf_agghead_destroy.argtypes = None, [vp]
    L.gdf_agghead_forward.restype, L.gdf_agghead_forward.argtypes = ci, [vp, vp, ci, vp, vp]
    L.gdf_agghead_wgrad_workspace.restype, L.gdf_agghead_wgrad_workspace.argtypes = C.c_size_t, [ci] * 5
    L.gdf_agghead_wgrad.restype, L.gdf_agghead_wgrad.argtypes = ci, [vp, ci, vp, ci, vp, ci, vp, C.c_size_t, vp]
    L.gdf_last_error.restype = C.c_char_p
    return L


def gen_grad(B, Cout, H, W, seed, heavy=False):
    """(B, Cout, H, W) fp32 contiguous"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, Cout, H, W, generator=g)
    if heavy:
        return (v * 2.0 ** (-30 * torch.rand(B, Cout, H, W, generator=g)) * 1e-4).float().contiguous()
    return (v * 1e-5).float().contiguous()


def wgrad(x, g, dtype):
    """the weight gradient of F.conv2d(x, w, padding=1) for the output gradient g, computed in `dtype` on the CPU -> (Cout, Cin, 3, 3)"""
    return torch.nn.grad.conv2d_weight(x.to(dtype), (g.shape[1], x.shape[1], 3, 3), g.to(dtype), padding=1)


def oracle(x, g):
    return wgrad(x, g, torch.float64)


def reference(x, g):
    return wgrad(x, g, torch.float32)


def channel_rel(got, want):
    """(Cout, Cin, 3, 3) -> (Cin,) relative L2 error per input channel against the float64 oracle; a channel whose oracle is all zero is 0 when
    the result is all zero there and inf otherwise"""
    d = (got.double() - want).pow(2).sum((0, 2, 3)).sqrt()
    n = want.pow(2).sum((0, 2, 3)).sqrt()
    rel = d / n
    return torch.where(n == 0, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))), rel)


def channel_error(got, want):
    rel = channel_rel(got, want)
    return float(rel.max()) if bool(torch.isfinite(rel).all()) else float("inf")


class Bounds:
    """the bound of one case, taken from the reference's fp32 arithmetic on that case's inputs"""

    def __init__(self, x, g):
        self.oracle = oracle(x, g)
        self.ref_err = channel_error(reference(x, g), self.oracle)
        self.bound = MARGIN * self.ref_err

    def check(self, got, what=""):
        assert tuple(got.shape) == tuple(self.oracle.shape), (what, tuple(got.shape), tuple(self.oracle.shape))
        err = channel_error(got, self.oracle)
        print("head weight gradient %s: worst channel error %.3e, bound %.3e (reference fp32: %.3e)" % (what, err, self.bound, self.ref_err))
        assert err <= self.bound, (what, err, self.bound)
        return err


# name: (Cin, Cout, B, H, W, fp32 map, channels-last, heavy-tailed G)
CASES = {
    "C8 -> 5, 6x6": (8, 5, 1, 6, 6, 0, 0, 0),                               # K = 36: less than one of anything
    "C72 -> 36, B2 9x7": (72, 36, 2, 9, 7, 0, 0, 0),                        # K tail, partial row and column blocks; image 1 follows image 0's last pixel
    "one row": (40, 7, 1, 1, 37, 0, 0, 0),                                  # every vertical tap in the padding, two patches along x
    "one column": (40, 7, 1, 37, 1, 0, 1, 0),                               # every horizontal tap in the padding
    "one pixel": (40, 7, 2, 1, 1, 0, 0, 0),
    "C200 -> 72, 17x16 channels-last": (200, 72, 2, 17, 16, 0, 1, 0),
    "C8 -> 5 fp32 NCHW": (8, 5, 1, 6, 6, 1, 0, 0),                          # the three-pass path
    "C136 -> 40 fp32 channels-last": (136, 40, 2, 12, 12, 1, 1, 0),
    "Cout 257": (24, 2 * ROWS + 1, 1, 8, 9, 0, 0, 0),                       # three row blocks, a one-row tail
    "one pixel over a patch each way": (16, 8, 1, PH + 1, PW + 1, 0, 0, 0),
    "heavy-tailed G": (72, 36, 2, 9, 7, 0, 0, 1),
    "C3520 -> 8, 8x8": (3520, 8, 1, 8, 8, 0, 0, 0),                         # the reference's column count: 110 channel tiles
    "C24 -> 16, 128x128": (24, 16, 1, 128, 128, 0, 0, 0),                   # the reference's full K: the accumulation-depth case
    "C24 -> 16, 128x128 B2": (24, 16, 2, 128, 128, 0, 0, 0),
}


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x (in its layout), G, Bounds) of a case; computed once and shared (never modified)"""
    Cin, Cout, B, H, W, f32, chlast, heavy = CASES[name]
    seed = sum(map(ord, name))
    x = gen_features(B, Cin, H, W, bool(f32), seed + 1)
    g = gen_grad(B, Cout, H, W, seed + 2, bool(heavy))
    return (_cl(x) if chlast else x), g, Bounds(x, g)


def emulate(x, g):
    """the kernel's split arithmetic on the CPU: every output channel of G scaled by the power of two that puts its maximum into [2^13, 2^14),
    an fp16 (hi, lo) pair per element (saturating), an fp32 map split likewise, the passes lo x, (hi x_lo,) hi x accumulated in fp32 (torch's
    CPU summation order, not the kernel's), the scale undone exactly -> (Cout, Cin, 3, 3) fp32"""
    mx = g.abs().amax((0, 2, 3))
    sh = torch.where((mx > 0) & torch.isfinite(mx), 13 - torch.frexp(mx)[1] + 1, torch.zeros_like(mx, dtype=torch.int32)).to(torch.int32)
    gs = torch.ldexp(g, sh[None, :, None, None])

    def split(v):
        hi = v.clamp(-65504, 65504).half().float()
        return hi, (v - hi).clamp(-65504, 65504).half().float()
    ghi, glo = split(gs)
    if x.dtype == torch.float32:
        xhi, xlo = split(x)
        acc = wgrad(xhi, glo, torch.float32) + wgrad(xlo, ghi, torch.float32) + wgrad(xhi, ghi, torch.float32)
    else:
        acc = wgrad(x, glo, torch.float32) + wgrad(x, ghi, torch.float32)
    return torch.ldexp(acc, -sh[:, None, None, None])


# ------------------------------------------------------------------------------------------------------------------------------
# one training step and a short run: the chain conv -> clip loss -> backward in a given precision on the CPU
# ------------------------------------------------------------------------------------------------------------------------------
STEP = dict(Cin=8, Cout=8, H=12, W=12, N=20, seed=4242)


@functools.lru_cache(maxsize=None)
def step_inputs():
    """-> (w (8, 8, 3, 3) fp32, x1, x2 (1, 8, 12, 12) fp16, src, tgt (1, N) int64)"""
    import clip_loss_ref as CR
    s = STEP
    w, _ = gen_weight(s["Cout"], s["Cin"], s["seed"])
    x1 = CR.features(1, s["Cin"], s["H"], s["W"], False, s["seed"] + 1, smoothed=True)
    x2 = CR.features(1, s["Cin"], s["H"], s["W"], False, s["seed"] + 2, smoothed=True)
    P = s["H"] * s["W"]
    return w, x1, x2, CR.indices(1, s["N"], P, s["seed"] + 3, distinct=True), CR.indices(1, s["N"], P, s["seed"] + 4, distinct=True)


def chain_grad(w, x1, x2, src, tgt, dtype):
    """-> (loss, d loss / d w) of conv -> compute_clip_loss in `dtype` on the CPU (fp32: both similarity matrices, as the reference)"""
    import clip_loss_ref as CR
    wt = w.detach().to(dtype).clone().requires_grad_(True)
    a, b = F.conv2d(x1.to(dtype), wt, padding=1), F.conv2d(x2.to(dtype), wt, padding=1)
    loss = CR._chain_loss(a, b, src, tgt, CR.SCALE, dtype == torch.float32)
    loss.backward()
    return loss.detach(), wt.grad


@functools.lru_cache(maxsize=None)
def step_bounds():
    """-> (oracle gradient fp64, bound): MARGIN x the worst channel of the fp32 CPU chain against the fp64 chain"""
    w, x1, x2, src, tgt = step_inputs()
    want = chain_grad(w, x1, x2, src, tgt, torch.float64)[1]
    ref_err = channel_error(chain_grad(w, x1, x2, src, tgt, torch.float32)[1], want)
    return want, MARGIN * ref_err, ref_err


RUN = dict(Cin=8, Cout=8, H=12, W=12, N=24, seed=77, steps=20)


@functools.lru_cache(maxsize=None)
def run_inputs():
    """one planted pair: the second map is the first rolled by (2, 3) pixels plus a little noise, and the annotated points correspond"""
    import clip_loss_ref as CR
    s = RUN
    x1 = CR.features(1, s["Cin"], s["H"], s["W"], True, s["seed"], smoothed=True)
    g = torch.Generator().manual_seed(s["seed"] + 1)
    x2 = torch.roll(x1, (2, 3), (2, 3)) + 0.05 * torch.randn(x1.shape, generator=g)
    src = CR.indices(1, s["N"], s["H"] * s["W"], s["seed"] + 2, distinct=True)
    y, x = src // s["W"], src % s["W"]
    tgt = ((y + 2) % s["H"]) * s["W"] + (x + 3) % s["W"]
    return x1.half(), x2.half(), src, tgt


def training_run(head, loss_fn, x1, x2, src, tgt, steps=None):
    """the reference's loop on one pair: AdamW(lr=5e-4, weight_decay=0.01) -> the loss before every step, and after the last"""
    opt = torch.optim.AdamW(head.parameters(), lr=5e-4, weight_decay=0.01)
    losses = []
    for _ in range(steps or RUN["steps"]):
        opt.zero_grad()
        loss = loss_fn(head(x1), head(x2), src, tgt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(loss_fn(head(x1), head(x2), src, tgt)))
    return losses


def run_head():
    """a fresh head for the run: the same seeded initialisation wherever it is built"""
    w, _ = gen_weight(RUN["Cout"], RUN["Cin"], RUN["seed"] + 5)
    return w
